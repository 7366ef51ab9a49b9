"""OpenFOAM ASCII case files <-> the flat arrays of the C-ABI.

Readers and writers for ``constant/polyMesh/{points,faces,owner,neighbour,boundary}``,
``vol{Scalar,Vector}Field`` files of a time directory, and the handful of dictionary
entries QGDFoam reads (QGDFoam/createFields.H, thermophysicalProperties, fvSchemes
``fvsc`` [fvsc.C L47-58], controlDict), so that a case prepared for the reference
solver can be loaded into a ``QGDFoamCase`` and its result written back.

The same for the QHD family: ``read_qhd_case_setup`` / ``read_srf_case_setup`` / ``read_scalar_case_setup`` (their common thermo block is
``_read_qhd_thermo``, every reader's walk over fvSolution.solvers ``_solver_entries``), ``assemble_qhd_case`` / ``assemble_scalar_case``
(what a reader returned -> Device and case; ``load_*`` and the applications call them), and the writers ``write_time``,
``write_cell_fields``, ``write_qhd_time``, ``write_srf_time``, ``write_scalar_time``, ``write_species_fields``, which share one patch
table (``_patch_table``).  ``read_run_control`` is controlDict's run control for ``apprun.run_control``.

Only the ASCII stream format is handled (``format binary`` is refused loudly).
The file grammar is OpenFOAM's (L0: OpenFOAM itself is not part of the reference
tree); nothing in here is on the timed path.
"""
import os
import re

import numpy as np

from . import _lib as L
from .mesh import PolyMesh

# OpenFOAM v2312 universal gas constant [J/(kmol K)] (L0 assumption: 1000 * physicoChemical::R)
RR = 8314.46261815324

PATCH_TYPES = {
    "patch": L.PATCH_GENERIC, "wall": L.PATCH_GENERIC, "empty": L.PATCH_EMPTY, "symmetryPlane": L.PATCH_SYMMETRYPLANE,
    "symmetry": L.PATCH_SYMMETRY, "wedge": L.PATCH_WEDGE, "cyclic": L.PATCH_CYCLIC,
}
PATCH_WORDS = {L.PATCH_GENERIC: "patch", L.PATCH_EMPTY: "empty", L.PATCH_SYMMETRYPLANE: "symmetryPlane",
               L.PATCH_SYMMETRY: "symmetry", L.PATCH_WEDGE: "wedge", L.PATCH_CYCLIC: "cyclic"}
_CONSTRAINT_BCS = {"empty", "symmetryPlane", "symmetry", "wedge", "cyclic"}


class FoamFileError(ValueError):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# tokenizer / dictionary parser
# ---------------------------------------------------------------------------------------------------------------------
_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
_TOKEN = re.compile(r'\s*("(?:[^"\\]|\\.)*"|[{}()\[\];]|[^\s{}()\[\];"]+)')
_LIST_HEAD = re.compile(r"(?:List<\s*(\w+)\s*>\s*)?(?<![\w.+-])(\d+)\s*\(")


def _strip_comments(text):
    return _COMMENT.sub(" ", text)


def _number(tok):
    try:
        return int(tok)
    except ValueError:
        try:
            return float(tok)
        except ValueError:
            return tok


_WORD_START = re.compile(r"[A-Za-z_]")
_WORD_END = set(" \t\r\n;{}[]\"")


def _tokenize(text):
    """OpenFOAM's token stream as far as dictionaries need it.  A word that starts with a letter runs on through BALANCED parentheses
    (ISstream::read(word&), L0): `grad(U)`, `div(phiJm,U)`, `interpolate((U*rhoU))` are single keywords; a '(' at the start of a
    token, or after a number (`4(a b c d)`), is punctuation."""
    toks = []
    pos, n = 0, len(text)
    while pos < n:
        m = _TOKEN.match(text, pos)
        if m is None:
            pos += 1
            continue
        tok = m.group(1)
        start, end = m.start(1), m.end()
        if _WORD_START.match(tok) and end < n and text[end] == "(":
            depth, k = 0, end
            while k < n:
                ch = text[k]
                if ch == "(":
                    depth += 1
                elif ch == ")":
                    if depth == 0:
                        break
                    depth -= 1
                elif ch in _WORD_END:
                    break
                k += 1
            if depth == 0:   # balanced: the parentheses belong to the word
                tok, end = text[start:k], k
        toks.append(tok)
        pos = end
    return toks


class _Parser:
    def __init__(self, text, lists):
        self.toks = _tokenize(text)
        self.i = 0
        self.lists = lists

    def peek(self):
        return self.toks[self.i] if self.i < len(self.toks) else None

    def next(self):
        t = self.peek()
        if t is None:
            raise FoamFileError("unexpected end of file")
        self.i += 1
        return t

    def parse_dict_body(self, top=False):
        d = {}
        while True:
            t = self.peek()
            if t is None:
                if top:
                    return d
                raise FoamFileError("missing '}'")
            if t == "}":
                if top:
                    raise FoamFileError("unbalanced '}'")
                self.i += 1
                return d
            key = self.next()
            if key == ";":
                continue
            if key.startswith('"'):
                key = key[1:-1]
            if self.peek() == "{":
                self.i += 1
                d[key] = self.parse_dict_body()
                continue
            vals = []
            while self.peek() != ";":
                if self.peek() is None or self.peek() == "}":
                    raise FoamFileError(f"entry '{key}' is not terminated by ';'")
                vals.append(self.parse_value())
            self.i += 1
            d[key] = vals[0] if len(vals) == 1 else vals
        return d

    def parse_value(self):
        t = self.next()
        if t == "(":
            return self.parse_list()
        if t == "[":
            out = []
            while self.peek() != "]":
                out.append(_number(self.next()))
            self.i += 1
            return ("dimensions", out)
        if t == "{":
            return self.parse_dict_body()
        if t.startswith("@LIST"):
            return self.lists[int(t[5:])]
        if t.startswith('"'):
            return t[1:-1]
        # "N(" and "List<T> N (" prefixes of short in-line lists
        if re.fullmatch(r"\d+", t) and self.peek() == "(":
            self.i += 1
            return self.parse_list()
        if re.fullmatch(r"List<\w+>", t):
            return self.parse_value()
        return _number(t)

    def parse_list(self):
        out = []
        while self.peek() != ")":
            if self.peek() is None:
                raise FoamFileError("missing ')'")
            out.append(self.parse_value())
        self.i += 1
        return out


def _extract_big_lists(text, min_items=64):
    """Replace long numeric lists ``N ( ... )`` by @LISTk placeholders, parsed with numpy."""
    lists = []
    out = []
    pos = 0
    for m in _LIST_HEAD.finditer(text):
        if m.start() < pos:
            continue
        n = int(m.group(2))
        if n < min_items:
            continue
        start = m.end()
        # depth of the items: scalar list "1 2 3", or nested "(x y z)" / "4(a b c d)"
        k = start
        while k < len(text) and text[k].isspace():
            k += 1
        nested = k < len(text) and (text[k] == "(" or re.match(r"\d+\s*\(", text[k:k + 24]) is not None)
        if nested:
            e = re.compile(r"\)\s*\)").search(text, start)
            if e is None:
                raise FoamFileError("unterminated list")
            end = e.end() - 1
        else:
            end = text.find(")", start)
            if end < 0:
                raise FoamFileError("unterminated list")
        body = text[start:end]
        ragged = nested and text[k] != "("
        try:
            flat = np.array(body.replace("(", " ").replace(")", " ").split(), dtype=np.float64)
        except ValueError:
            continue  # not a numeric list (e.g. a boundary file with 64 or more patches): left to the token parser
        if ragged:
            lists.append(("ragged", n, flat))
        elif nested:
            if flat.size % n:
                raise FoamFileError("list length does not match its header")
            lists.append(flat.reshape(n, flat.size // n))
        else:
            if flat.size != n:
                raise FoamFileError(f"list of {flat.size} items announced as {n}")
            lists.append(flat)
        out.append(text[pos:m.start()])
        out.append(f" @LIST{len(lists) - 1} ")
        pos = end + 1
    out.append(text[pos:])
    return "".join(out), lists


def parse_foam_text(text):
    """Parse an OpenFOAM dictionary-style file into nested dicts (lists -> python lists / numpy arrays)."""
    text = _strip_comments(text)
    text, lists = _extract_big_lists(text)
    p = _Parser(text, lists)
    d = p.parse_dict_body(top=True)
    hdr = d.get("FoamFile", {})
    if isinstance(hdr, dict) and str(hdr.get("format", "ascii")) != "ascii":
        raise FoamFileError("only 'format ascii' files are supported")
    return d


def _read_text(path):
    """text of a case file; OpenFOAM's writeCompression leaves <name>.gz instead of <name>"""
    if not os.path.exists(path) and os.path.exists(path + ".gz"):
        import gzip
        with gzip.open(path + ".gz", "rt") as f:
            return f.read()
    with open(path) as f:
        return f.read()


def _exists(path):
    return os.path.exists(path) or os.path.exists(path + ".gz")


def read_dict(path):
    return parse_foam_text(_read_text(path))


# function objects of system/controlDict the QGDFoam application serves (monitor.FunctionObjects): type -> the fields it may name
# (probes and fieldMinMax also take the names of the case's species; qgdSpeciesIntegrals and qgdSpeciesPatchFluxes need a case with species)
FUNCTION_TYPES = {"probes": ("rho", "U", "p", "T", "e"), "fieldMinMax": ("rho", "p", "T", "U", "mag(U)", "Mach"), "qgdIntegrals": (),
                  "qgdPatchFluxes": (), "qgdSpeciesIntegrals": (), "qgdSpeciesPatchFluxes": ()}
SPECIES_FUNCTION_TYPES = ("qgdSpeciesIntegrals", "qgdSpeciesPatchFluxes")


def read_functions(control_dict, warn=print, species=None):
    """specifications of the served entries of ``functions{}``: a list of dict(name, type, interval, fields, probeLocations, patches).
    ``probes`` (fields out of rho U p T e, probeLocations), ``fieldMinMax`` (fields out of rho p T U Mach; U is its magnitude),
    and the project's own ``qgdIntegrals`` and ``qgdPatchFluxes`` (patches) are served, each every ``writeInterval`` steps
    (``writeControl timeStep``, the default; default interval 1).  Anything else -- another type, another writeControl, a field a
    type does not serve -- gets one warning line and is skipped, so that a case with functions the solver does not know still runs.
    ``species``: the names of the case's species (None or empty: it carries none).  ``probes`` and ``fieldMinMax`` then take species names
    in ``fields`` next to the flow fields, and ``qgdSpeciesIntegrals`` and ``qgdSpeciesPatchFluxes`` (patches) are served; in a case
    without species those two types are an error that names the function (a species name among ``fields`` is then just a field that is
    not served: warned about by name and left out, as any unknown field is)."""
    return _read_functions(control_dict, warn, FUNCTION_TYPES, ("qgdPatchFluxes", "qgdSpeciesPatchFluxes"), species)


# the function objects the QHDFoam and SRFQHDFoam applications serve (monitor.QHDFunctionObjects): type -> the fields it may name
QHD_FUNCTION_TYPES = {"probes": ("U", "T", "p"), "fieldMinMax": ("U", "mag(U)", "T", "p", "contErr"), "qhdIntegrals": (), "qhdPatchFluxes": (),
                      "qhdContinuityErrors": ()}


def read_qhd_functions(control_dict, warn=print):
    """``read_functions`` for a QHDFoam or SRFQHDFoam case: ``probes`` (fields out of U T p, probeLocations), ``fieldMinMax`` (fields out
    of U T p contErr; U is its magnitude, contErr is |sum of phi over the cell's faces| / V), and the project's own ``qhdIntegrals``,
    ``qhdPatchFluxes`` (patches) and ``qhdContinuityErrors``, each every ``writeInterval`` steps.  Anything else gets one warning line
    that names it and is skipped."""
    return _read_functions(control_dict, warn, QHD_FUNCTION_TYPES, ("qhdPatchFluxes",), None)


def _read_functions(control_dict, warn, types, patch_types, species):
    """the parsing read_functions and read_qhd_functions share: ``types`` maps a served type to the fields it may name, ``patch_types``
    are the types that need ``patches``"""
    species = [str(n) for n in (species or [])]
    funcs = control_dict.get("functions", {})
    out = []
    if not isinstance(funcs, dict):
        return out
    for name, d in funcs.items():
        if not isinstance(d, dict):
            continue
        typ = str(d.get("type", ""))
        if typ not in types:
            warn(f"functions: '{name}' has type '{typ}', which is not served (served: {', '.join(types)}): skipped")
            continue
        if not _truthy(d.get("enabled", "yes")):
            continue
        control = str(d.get("writeControl", d.get("outputControl", "timeStep")))
        if control != "timeStep":
            warn(f"functions: '{name}': writeControl '{control}' is not served (timeStep is): skipped")
            continue
        interval = int(d.get("writeInterval", d.get("outputInterval", 1)))
        if interval < 1:
            raise FoamFileError(f"functions: '{name}': writeInterval must be at least 1, got {interval}")
        if typ in SPECIES_FUNCTION_TYPES and not species:
            raise FoamFileError(f"functions: '{name}': type {typ} needs a case with species (thermophysicalProperties lists none)")
        spec = dict(name=str(name), type=typ, interval=interval)
        if types[typ]:
            fields = d.get("fields", [])
            fields = [str(f) for f in (fields if isinstance(fields, (list, tuple)) else [fields])]
            can = types[typ] + tuple(n for n in species if n not in types[typ])
            served = [f for f in fields if f in can]
            for f in fields:
                if f not in served:
                    warn(f"functions: '{name}': field '{f}' is not served by type {typ} (served: {', '.join(can)}): left out")
            if not served:
                warn(f"functions: '{name}': no served field: skipped")
                continue
            spec["fields"] = served
        if typ == "probes":
            locs = d.get("probeLocations")
            try:
                locs = np.asarray(locs, dtype=np.float64).reshape(-1, 3)
            except (TypeError, ValueError):
                raise FoamFileError(f"functions: '{name}': probeLocations must be a list of points (x y z)") from None
            if locs.shape[0] == 0:
                warn(f"functions: '{name}': no probeLocations: skipped")
                continue
            spec["probeLocations"] = locs
        if typ in patch_types:
            patches = d.get("patches", [])
            patches = [str(p) for p in (patches if isinstance(patches, (list, tuple)) else [patches])]
            if not patches:
                warn(f"functions: '{name}': no patches: skipped")
                continue
            spec["patches"] = patches
        out.append(spec)
    return out


def _split_header(text):
    """(FoamFile dict, rest of the text) of a list-style file (points, faces, owner, ...)"""
    text = _strip_comments(text)
    m = re.search(r"FoamFile\s*\{", text)
    hdr = {}
    if m:
        end = text.index("}", m.end())
        hdr = _Parser(text[m.end():end], []).parse_dict_body(top=True)
        text = text[end + 1:]
    if str(hdr.get("format", "ascii")) != "ascii":
        raise FoamFileError("only 'format ascii' files are supported")
    return hdr, text


def _read_list_file(path):
    hdr, text = _split_header(_read_text(path))
    m = _LIST_HEAD.search(text)
    if m is None:
        raise FoamFileError(f"{path}: no list found")
    n = int(m.group(2))
    body = text[m.end():text.rindex(")")]
    flat = np.array(body.replace("(", " ").replace(")", " ").split(), dtype=np.float64)
    return hdr, n, flat


# ---------------------------------------------------------------------------------------------------------------------
# polyMesh
# ---------------------------------------------------------------------------------------------------------------------
def read_polymesh(poly_dir):
    """constant/polyMesh -> PolyMesh (with ``patch_names``).  processor patches are refused: a decomposed case is
    loaded whole and sharded by cell ranges instead (multi-GPU)."""
    _, npnt, flat = _read_list_file(os.path.join(poly_dir, "points"))
    if flat.size != 3 * npnt:
        raise FoamFileError("points: size mismatch")
    points = flat
    _, nf, flat = _read_list_file(os.path.join(poly_dir, "faces"))
    ints = flat.astype(np.int64)
    if ints.size == 5 * nf and np.all(ints[0::5] == 4):
        sizes = np.full(nf, 4, dtype=np.int64)
        fp = ints.reshape(nf, 5)[:, 1:].reshape(-1)
    else:
        sizes = np.empty(nf, dtype=np.int64)
        keep = np.ones(ints.size, dtype=bool)
        k = 0
        for f in range(nf):
            s = ints[k]
            sizes[f] = s
            keep[k] = False
            k += s + 1
        if k != ints.size:
            raise FoamFileError("faces: size mismatch")
        fp = ints[keep]
    fo = np.zeros(nf + 1, dtype=np.int64)
    np.cumsum(sizes, out=fo[1:])
    hdr_o, no, owner = _read_list_file(os.path.join(poly_dir, "owner"))
    _, nn, neighbour = _read_list_file(os.path.join(poly_dir, "neighbour"))
    if no != nf or owner.size != nf or neighbour.size != nn:
        raise FoamFileError("owner/neighbour: size mismatch")
    owner = owner.astype(np.int32)
    neighbour = neighbour.astype(np.int32)
    n_cells = int(owner.max()) + 1 if nf else 0
    note = str(hdr_o.get("note", ""))
    m = re.search(r"nCells:\s*(\d+)", note)
    if m:
        n_cells = int(m.group(1))

    _, text = _split_header(_read_text(os.path.join(poly_dir, "boundary")))
    m = re.search(r"(\d+)\s*\(", text)
    if m is None:
        raise FoamFileError("boundary: no patch list")
    body = text[m.end():text.rindex(")")]
    pd = _Parser(body, []).parse_dict_body(top=True)
    if len(pd) != int(m.group(1)):
        raise FoamFileError("boundary: patch count mismatch")
    names, start, size, ptype, partner = [], [], [], [], {}
    for name, e in pd.items():
        t = str(e.get("type", "patch"))
        if t not in PATCH_TYPES:
            raise FoamFileError(f"boundary: patch '{name}' of type '{t}' is not supported")
        names.append(name)
        start.append(int(e["startFace"]))
        size.append(int(e["nFaces"]))
        ptype.append(PATCH_TYPES[t])
        if t == "cyclic" and "neighbourPatch" in e:
            partner[name] = str(e["neighbourPatch"])
            if str(e.get("transform", "unknown")) == "rotational":
                raise FoamFileError(f"boundary: cyclic patch '{name}' is rotational: only translational cyclic pairs are served")
    mesh = PolyMesh.from_arrays(points, fo, fp, owner, neighbour, n_cells, start, size, ptype)
    mesh.patch_names = names
    # cyclic pairs (patch index of a half, of its neighbourPatch), each pair once, in patch order: what PolyMesh.unroll_cyclic takes
    mesh.cyclic_pairs = []
    for i, name in enumerate(names):
        if name in partner:
            other = partner[name]
            if other not in names or partner.get(other) != name:
                raise FoamFileError(f"boundary: cyclic patch '{name}' names neighbourPatch '{other}', which does not name it back")
            j = names.index(other)
            if i < j:
                mesh.cyclic_pairs.append((i, j))
    # the faceSet the leastSquares stencil reads if present [leastSquaresStencil.C L63-70]
    dsf = os.path.join(poly_dir, "sets", "degenerateStencilFaces")
    if _exists(dsf):
        _, nset, labels = _read_list_file(dsf)
        if labels.size != nset:
            raise FoamFileError("sets/degenerateStencilFaces: size mismatch")
        mesh.set_degenerate_faces(labels.astype(np.int32))
    return mesh


def _header(cls, obj, location, note=None):
    lines = ["FoamFile", "{", "    version     2.0;", "    format      ascii;", f"    class       {cls};"]
    if note:
        lines.append(f'    note        "{note}";')
    lines += [f'    location    "{location}";', f"    object      {obj};", "}", ""]
    return "\n".join(lines) + "\n"


def _fmt(x):
    return repr(float(x))


def write_polymesh(mesh, poly_dir, patch_names=None):
    """PolyMesh -> constant/polyMesh (ASCII, full-precision reals so a round trip is bit-exact)."""
    os.makedirs(poly_dir, exist_ok=True)
    names = patch_names or getattr(mesh, "patch_names", None) or [f"patch{i}" for i in range(mesh.nPatches)]
    pts = mesh.array("points").reshape(-1, 3)
    fo = mesh.array("faceOffsets")
    fp = mesh.array("facePoints")
    owner = mesh.array("owner")
    neighbour = mesh.array("neighbour")
    note = f"nPoints:{mesh.nPoints}  nCells:{mesh.nCells}  nFaces:{mesh.nFaces}  nInternalFaces:{mesh.nInternalFaces}"
    with open(os.path.join(poly_dir, "points"), "w") as f:
        f.write(_header("vectorField", "points", "constant/polyMesh"))
        f.write(f"{mesh.nPoints}\n(\n")
        f.write("\n".join(f"({_fmt(p[0])} {_fmt(p[1])} {_fmt(p[2])})" for p in pts))
        f.write("\n)\n")
    with open(os.path.join(poly_dir, "faces"), "w") as f:
        f.write(_header("faceList", "faces", "constant/polyMesh"))
        f.write(f"{mesh.nFaces}\n(\n")
        f.write("\n".join(f"{fo[i + 1] - fo[i]}({' '.join(map(str, fp[fo[i]:fo[i + 1]]))})" for i in range(mesh.nFaces)))
        f.write("\n)\n")
    for name, arr in (("owner", owner), ("neighbour", neighbour)):
        with open(os.path.join(poly_dir, name), "w") as f:
            f.write(_header("labelList", name, "constant/polyMesh", note))
            f.write(f"{arr.size}\n(\n")
            f.write("\n".join(map(str, arr)))
            f.write("\n)\n")
    ps, pz, pt = mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")
    with open(os.path.join(poly_dir, "boundary"), "w") as f:
        f.write(_header("polyBoundaryMesh", "boundary", "constant/polyMesh"))
        f.write(f"{mesh.nPatches}\n(\n")
        for i in range(mesh.nPatches):
            if int(pt[i]) not in PATCH_WORDS:
                raise FoamFileError("halo (cell-range shard) patches have no polyMesh spelling")
            nbr = ""
            for pa, pb in getattr(mesh, "cyclic_pairs", []):
                if i in (pa, pb):
                    nbr = f"        neighbourPatch  {names[pb if i == pa else pa]};\n"
            f.write(f"    {names[i]}\n    {{\n        type            {PATCH_WORDS[int(pt[i])]};\n{nbr}"
                    f"        nFaces          {int(pz[i])};\n        startFace       {int(ps[i])};\n    }}\n")
        f.write(")\n")


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
def _field_values(v, n, ncomp, what):
    """'uniform x' / 'nonuniform List<T> N (...)' entry -> (n, ncomp) array"""
    if isinstance(v, list) and len(v) == 2 and v[0] == "uniform":
        val = np.asarray(v[1], dtype=np.float64).reshape(-1)
        if val.size != ncomp:
            raise FoamFileError(f"{what}: uniform value has {val.size} components, expected {ncomp}")
        return np.tile(val, (n, 1))
    if isinstance(v, list) and len(v) >= 2 and v[0] == "nonuniform":
        arr = np.asarray(v[-1], dtype=np.float64)
        if arr.size != n * ncomp:
            raise FoamFileError(f"{what}: {arr.size} values for {n} x {ncomp}")
        return arr.reshape(n, ncomp)
    raise FoamFileError(f"{what}: cannot read value '{v}'")


def read_field(path, mesh):
    """vol<Type>Field file -> (internal (nCells, ncomp) array, {patch name: {'type': word, 'value': array|None, ...}})"""
    d = read_dict(path)
    cls = str(d.get("FoamFile", {}).get("class", ""))
    ncomp = {"volScalarField": 1, "volVectorField": 3}.get(cls)
    if ncomp is None:
        raise FoamFileError(f"{path}: class '{cls}' is not a vol scalar/vector field")
    internal = _field_values(d["internalField"], mesh.nCells, ncomp, f"{path}: internalField")
    names = getattr(mesh, "patch_names", None) or [f"patch{i}" for i in range(mesh.nPatches)]
    sizes = mesh.array("patchSize")
    bf = d.get("boundaryField", {})
    patches = {}
    for i, name in enumerate(names):
        e = bf.get(name)
        if e is None:  # OpenFOAM also accepts regular-expression keys
            for k, v in bf.items():
                try:
                    if re.fullmatch(k, name):
                        e = v
                        break
                except re.error:
                    pass
        if e is None:
            raise FoamFileError(f"{path}: no boundaryField entry for patch '{name}'")
        rec = dict(e)
        rec["type"] = str(e["type"])
        rec["value"] = _field_values(e["value"], int(sizes[i]), ncomp, f"{path}: {name}.value") if "value" in e else None
        if "gradient" in e:   # fixedGradient / qhdFlux patches
            rec["gradient"] = _field_values(e["gradient"], int(sizes[i]), ncomp, f"{path}: {name}.gradient")
        patches[name] = rec
    return internal, patches


def write_field(path, mesh, name, internal, patches, dimensions="[0 0 0 0 0 0 0]"):
    """(nCells[, 3]) array + {patch: (type word, value or None[, {extra entry: scalar}])} -> vol<Type>Field file (values at full
    precision; the optional third member writes further uniform entries of the patch, e.g. the gradient of a fixedGradient patch)"""
    a = np.asarray(internal, dtype=np.float64)
    vec = a.ndim == 2 and a.shape[1] == 3
    cls, typ = ("volVectorField", "vector") if vec else ("volScalarField", "scalar")

    def one(x):
        return f"({_fmt(x[0])} {_fmt(x[1])} {_fmt(x[2])})" if vec else _fmt(x)

    def values(arr):
        arr = np.asarray(arr, dtype=np.float64)
        if arr.ndim == (1 if vec else 0):
            return f"uniform {one(arr)}"
        return f"nonuniform List<{typ}> {len(arr)}\n(\n" + "\n".join(one(x) for x in arr) + "\n)"

    names = getattr(mesh, "patch_names", None) or [f"patch{i}" for i in range(mesh.nPatches)]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(_header(cls, name, os.path.basename(os.path.dirname(path))))
        f.write(f"dimensions      {dimensions};\n\ninternalField   {values(a)};\n\nboundaryField\n{{\n")
        for pn in names:
            t, v = patches[pn][0], patches[pn][1]
            f.write(f"    {pn}\n    {{\n        type            {t};\n")
            for key, x in (patches[pn][2].items() if len(patches[pn]) > 2 else ()):
                f.write(f"        {key:<15} uniform {_fmt(float(x))};\n")
            if v is not None:
                f.write(f"        value           {values(v)};\n")
            f.write("    }\n")
        f.write("}\n")


# dimensions of the written fields; the p of the QHD family is kinematic
_DIMS = {"U": "[0 1 -1 0 0 0 0]", "T": "[0 0 0 1 0 0 0]", "p": "[1 -1 -2 0 0 0 0]", "rho": "[1 -3 0 0 0 0 0]", "ScQGD": "[0 0 0 0 0 0 0]"}
_QHD_DIMS = dict(_DIMS, p="[0 2 -2 0 0 0 0]")


def _patch_table(mesh, entry):
    """the ``patches`` of write_field for one field: a constraint patch is written as its own word, without a value; any other patch as
    entry(i, patch name, sl) -> (kind, value[, extra]), sl being the patch's slice of an array over the boundary faces"""
    names = getattr(mesh, "patch_names", None) or [f"patch{i}" for i in range(mesh.nPatches)]
    ps, pz, pt = mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")
    table = {}
    for i, pn in enumerate(names):
        word = PATCH_WORDS.get(int(pt[i]), "patch")
        b0 = int(ps[i]) - mesh.nInternalFaces
        table[pn] = (word, None) if word in _CONSTRAINT_BCS else entry(i, pn, slice(b0, b0 + int(pz[i])))
    return table


def _written_kind(bcs, i, fname):
    """the type word a resident case's writer gives patch i of field fname: the kind of its boundary condition, ``calculated`` where there
    is none"""
    kind = bcs[i][fname][0] if bcs is not None and fname in bcs[i] else "calculated"
    return "calculated" if kind == "none" else kind


# ---------------------------------------------------------------------------------------------------------------------
# case set-up (what QGDFoam's createFields.H reads)
# ---------------------------------------------------------------------------------------------------------------------
def _bc(rec, vector, patch_type_word, what, lists=False):
    """boundaryField entry -> the (kind, value) pair QGDFoamCase.set_bc takes.

    lists (the QGDFoam reader): a fixedValue entry written as `nonuniform List<scalar|vector>` comes back as the array of its values in
    patch-face order ((nFaces, 3) or (nFaces,)), `noSlip` on U is fixedValue (0 0 0); a value list on any other kind of entry is refused
    (the resident case would not evaluate it).  The QHDFoam and scalar readers keep to one value per patch.

    Constraint patches (L0: fvPatchField<Type>::New(p, iF, dict)): the entry's type must be the patch's own constraint type --
    OpenFOAM stops with "inconsistent patch and patchField types" otherwise -- and the field then IS that constraint field:
    symmetryPlane / symmetry reflect U (basicSymmetry, the library's ``slip`` arithmetic) and leave scalars zero-gradient; empty
    carries nothing.  cyclic / wedge fields are not served by the resident cases (read_case_setup refuses such meshes)."""
    t = rec["type"]
    if patch_type_word in _CONSTRAINT_BCS:
        if t != patch_type_word:
            raise FoamFileError(f"{what}: inconsistent patch and patchField types: the patch is '{patch_type_word}', the field says '{t}'")
        if patch_type_word == "empty":
            return ("none", None)
        if patch_type_word in ("symmetryPlane", "symmetry"):
            return ("slip", None) if vector else ("zeroGradient", None)
        if patch_type_word == "cyclic":
            return ("none", None)   # the pair's faces become internal faces (PolyMesh.unroll_cyclic): no patch field is left to evaluate
        raise FoamFileError(f"{what}: '{patch_type_word}' patch fields are not supported by the resident cases")
    if t in _CONSTRAINT_BCS:
        raise FoamFileError(f"{what}: boundary condition '{t}' needs a patch of that type (the patch is '{patch_type_word}')")
    if t in ("zeroGradient", "slip", "qgdFlux"):
        v = rec.get("value")
        if lists and v is not None and len(v) and np.any(v != v[0]):
            raise FoamFileError(f"{what}: a value list on a '{t}' entry is not supported (per-face values belong to fixedValue entries)")
        if t == "slip" and not vector:
            return ("zeroGradient", None)  # slip on a scalar is zeroGradient (basicSymmetry, L0)
        return (t, None)
    if t == "noSlip" and vector and lists:
        return ("fixedValue", np.zeros(3))   # noSlipFvPatchVectorField: fixedValue (0 0 0) without a value entry (L0)
    if t == "fixedValue":
        v = rec["value"]
        if v is None:
            raise FoamFileError(f"{what}: fixedValue needs a value")
        if len(v) and np.any(v != v[0]):
            if not lists:
                raise FoamFileError(f"{what}: only uniform fixedValue patches are supported")
            return ("fixedValue", np.array(v if vector else v[:, 0], dtype=np.float64))
        if not len(v):
            return ("fixedValue", np.zeros(3) if vector else 0.0)   # a patch without faces
        return ("fixedValue", v[0] if vector else float(v[0, 0]))
    raise FoamFileError(f"{what}: boundary condition '{t}' is not supported")


def _refuse_unserved_patches(mesh, case_dir, cyclic_ok=False):
    """wedge patches with faces: their rotated patch fields are not served by the resident cases (the fvsc operators of a Device do serve
    such meshes).  cyclic patches: QGDFoam's explicit branch serves translational pairs named by `neighbourPatch` (cyclic_ok; the
    application unrolls them into ghost cells, PolyMesh.unroll_cyclic); QHDFoam does not."""
    pt, pz = mesh.array("patchType"), mesh.array("patchSize")
    paired = {i for pr in getattr(mesh, "cyclic_pairs", []) for i in pr}
    for i, name in enumerate(mesh.patch_names):
        word = PATCH_WORDS.get(int(pt[i]), "patch")
        if word == "cyclic" and int(pz[i]) > 0 and cyclic_ok:
            if i not in paired:
                raise FoamFileError(f"{case_dir}: cyclic patch '{name}' has no neighbourPatch entry in constant/polyMesh/boundary")
            continue
        if word in ("cyclic", "wedge") and int(pz[i]) > 0:
            raise FoamFileError(f"{case_dir}: patch '{name}' is a {word} patch; the resident QGDFoam / QHDFoam cases do not serve "
                                f"{word} patch fields")


def _scheme_words(v):
    """a scheme entry as the list of its words: `linear;` -> ['linear'], `Gauss linear corrected;` -> ['Gauss','linear','corrected']"""
    return [str(x) for x in v] if isinstance(v, list) else [str(v)]


def _find_entry(d, key):
    """dictionary::found / lookup of OpenFOAM (L0): the literal key first, then the quoted (regular-expression) keys, last one first"""
    if not isinstance(d, dict):
        return None
    if key in d:
        return d[key]
    for k in reversed(list(d.keys())):
        if k == key or not any(ch in k for ch in ".*+?[]|^$\\"):
            continue
        try:
            if re.fullmatch(k, key):
                return d[k]
        except re.error:
            pass
    return None


def read_face_schemes(fs, flux_terms, grad_terms, what="system/fvSchemes"):
    """The fvSchemes sub-dictionaries the face-flux path consults, checked against what the library computes.

    * ``fvsc`` [fvsc.C L47-58]: the word of every term in ``grad_terms`` (its own entry, else ``default``), returned per term.  The
      QGDFoam case serves up to two distinct stencils (``qgd_case_options::termStencil``); what a caller cannot serve it refuses itself.
    * ``interpolationSchemes`` [QGDInterpolate.H L42-66]: a field with an ``interpolate(<name>)`` entry, or any field under a
      ``default`` other than ``none``, goes to ``fvc::interpolate``: with ``linear`` that is linearInterpolate = the numbers the
      library produces; anything else is refused, naming the entry.  The sub-dictionary must exist (``subDict`` is fatal otherwise).
    * ``divSchemes`` [QGDInterpolate.H L86-104]: a flux with an entry of its own name (``div(phiJm,U)`` ...) goes to ``fvc::flux``;
      ``Gauss linear`` is flux * linear(psi) = the default branch, ``Gauss upwind`` the in-register upwind branch of the face kernels
      (options ``fluxScheme*``); limited schemes are refused.  ``default`` is NOT consulted by qgdFlux (``found(fluxName)``).

    Returns ({gradient term: stencil word}, {flux term: 'linear' | 'upwind'})."""
    fvsc = fs.get("fvsc")
    if not isinstance(fvsc, dict):
        raise FoamFileError(f"{what}: sub-dictionary 'fvsc' is missing [fvsc.C L51]")
    words = {}
    for term in grad_terms:
        v = _find_entry(fvsc, term)
        if v is None:
            v = _find_entry(fvsc, "default")
            if v is None:
                raise FoamFileError(f"{what}: fvsc has neither '{term}' nor 'default' [fvsc.C L57]")
        words[term] = _scheme_words(v)[0]
    interp = fs.get("interpolationSchemes")
    if not isinstance(interp, dict):
        raise FoamFileError(f"{what}: sub-dictionary 'interpolationSchemes' is missing (qgdInterpolate looks it up, QGDInterpolate.H L44)")
    for key, v in interp.items():
        w = _scheme_words(v)
        if key == "default":
            if w not in (["none"], ["linear"]):
                raise FoamFileError(f"{what}: interpolationSchemes.default '{' '.join(w)}' is not supported: the face-flux path interpolates "
                                    f"linearly (accepted: none, linear)")
        elif w != ["linear"]:
            raise FoamFileError(f"{what}: interpolationSchemes.{key} '{' '.join(w)}' is not supported: the face-flux path interpolates "
                                f"linearly (accepted: linear)")
    div = fs.get("divSchemes")
    if not isinstance(div, dict):
        raise FoamFileError(f"{what}: sub-dictionary 'divSchemes' is missing (qgdFlux looks it up, QGDInterpolate.H L86)")
    flux = {}
    for term in flux_terms:
        v = _find_entry(div, term)
        if v is None:
            flux[term] = "linear"      # flux*psif [QGDInterpolate.H L104]
            continue
        w = _scheme_words(v)
        if w == ["Gauss", "linear"]:
            flux[term] = "linear"
        elif w == ["Gauss", "upwind"]:
            flux[term] = "upwind"
        else:
            raise FoamFileError(f"{what}: divSchemes.{term} '{' '.join(w)}' is not supported (accepted: Gauss linear, Gauss upwind)")
    return words, flux


def _check_fv_schemes(fs, mesh, need_laplacian, need_grad, what="system/fvSchemes", otherwise=""):
    """ddtSchemes / laplacianSchemes / gradSchemes as far as the path's fvm:: / fvc:: operators read them (L0): Euler; the uncorrected
    Gauss linear laplacian (a corrected one is the same operator on an orthogonal mesh and is accepted there); Gauss linear gradients"""
    ddt = fs.get("ddtSchemes", {})
    w = _scheme_words(ddt.get("default", "Euler")) if isinstance(ddt, dict) else ["Euler"]
    if w != ["Euler"]:
        raise FoamFileError(f"{what}: ddtSchemes.default '{' '.join(w)}' is not supported (the path is the explicit Euler step of the reference)")
    if need_laplacian:
        lap = fs.get("laplacianSchemes", {})
        for key, v in (lap.items() if isinstance(lap, dict) else ()):
            w = _scheme_words(v)
            ok = w[:2] == ["Gauss", "linear"] and len(w) == 3 and w[2] in ("uncorrected", "orthogonal", "corrected")
            if ok and w[2] == "corrected" and not _orthogonal(mesh):
                raise FoamFileError(f"{what}: laplacianSchemes.{key} 'Gauss linear corrected' on a non-orthogonal mesh: the explicit "
                                    f"non-orthogonal correction is not part of the path (accepted: Gauss linear uncorrected{otherwise})")
            if not ok:
                raise FoamFileError(f"{what}: laplacianSchemes.{key} '{' '.join(w)}' is not supported (accepted: Gauss linear uncorrected)")
    if need_grad:
        gs = fs.get("gradSchemes", {})
        for key, v in (gs.items() if isinstance(gs, dict) else ()):
            w = _scheme_words(v)
            if w != ["Gauss", "linear"]:
                raise FoamFileError(f"{what}: gradSchemes.{key} '{' '.join(w)}' is not supported (accepted: Gauss linear)")


def _orthogonal(mesh, tol=1e-12):
    """every internal face normal parallel to the line of its two cell centres (nonOrthCorrectionVectors = 0 to rounding)"""
    nif = mesh.nInternalFaces
    if nif == 0:
        return True
    Sf = mesh.array("Sf").reshape(-1, 3)[:nif]
    C = mesh.array("C").reshape(-1, 3)
    d = C[mesh.array("neighbour")] - C[mesh.array("owner")[:nif]]
    n = Sf / np.linalg.norm(Sf, axis=1)[:, None]
    corr = n - d / (n * d).sum(axis=1)[:, None]
    return bool(np.abs(corr).max() <= tol)


def read_case_setup(case_dir, time="0"):
    """Read an OpenFOAM QGDFoam case directory.

    Returns (mesh, options dict for ``default_options``, {'U','T','p'} internal arrays, per-patch BC triples).
    Entries read: constant/polyMesh; constant/thermophysicalProperties (mixture.specie.molWeight,
    thermodynamics.Cv|Cp, transport.mu/Pr; QGD{implicitDiffusion, QGDCoeffs constScPrModel1 | varScModel7, <model>Dict{ScQGD,PrQGD}} as in
    QGDThermo.C L48-82, QGDCoeffs.C L57-160, constScPrModel1.C L48-90; varScModel7 also cSc1, minSc, maxSc, constScCellSet
    (constant/polyMesh/sets/<name>), returned as options["varSc"] [varScModel7.C L77-158]); system/fvSchemes fvsc.default (fvsc.C L47-58);
    system/controlDict deltaT/adjustTimeStep/maxCo/maxDeltaT (setDeltaT-QGDQHD.H); system/fvSolution solvers.{U,e}
    tolerance/maxIter (implicitDiffusion only); <time>/{U,T,p}.
    """
    mesh = read_polymesh(os.path.join(case_dir, "constant", "polyMesh"))
    _refuse_unserved_patches(mesh, case_dir, cyclic_ok=True)
    opt = {}
    tp = read_dict(os.path.join(case_dir, "constant", "thermophysicalProperties"))
    tt = tp.get("thermoType", {})
    for key, want in (("equationOfState", "perfectGas"), ("transport", "const")):
        if isinstance(tt, dict) and key in tt and str(tt[key]) != want:
            raise FoamFileError(f"thermoType.{key} '{tt[key]}' is not supported (only {want})")
    species_names = [str(w) for w in tp["species"]] if "species" in tp else None
    mix = _species_mixture(tp, species_names) if species_names else tp["mixture"]
    R = RR / float(mix["specie"]["molWeight"])
    th = mix["thermodynamics"]
    opt["R"] = R
    opt["Cv"] = float(th["Cv"]) if "Cv" in th else float(th["Cp"]) - R
    opt["mu"] = float(mix["transport"]["mu"])
    opt["Pr"] = float(mix["transport"]["Pr"])
    qgd = tp["QGD"]
    # QGDThermo::read(): implicitDiffusion defaults to true when absent [QGDThermo.C L70-82]
    opt["implicitDiffusion"] = 1 if _truthy(qgd.get("implicitDiffusion", "true")) else 0
    # not a reference entry: selects the physically consistent explicit energy update (qgd_case_options::consistentEnergy)
    if "consistentEnergy" in qgd:
        opt["consistentEnergy"] = 1 if _truthy(qgd["consistentEnergy"]) else 0
    model = str(qgd["QGDCoeffs"])
    if model not in ("constScPrModel1", "varScModel7"):
        raise FoamFileError(f"QGDCoeffs '{model}' is not supported (served: constScPrModel1, varScModel7)")
    md = qgd.get(model + "Dict", qgd)  # QGDCoeffs::New: <type>Dict when present, else the QGD dict [QGDCoeffs.C L81-116]
    if model == "varScModel7":
        # ScQGD and PrQGD are dict.lookup()s [varScModel7.C L77-78]; cSc1 defaults to 1, minSc / maxSc to -1 (off); smoothCoeff, rC,
        # badQualitySc and maxAspectRatio are read by the reference and never used [L262-265]: accepted, ignored
        for k in ("ScQGD", "PrQGD"):
            if k not in md:
                raise FoamFileError(f"QGD.{model}: entry '{k}' is missing [varScModel7.C L77-78]")
            opt[k] = float(md[k])
        if getattr(mesh, "cyclic_pairs", None):
            raise FoamFileError(f"{case_dir}: a case with cyclic patches runs with uniform alphaQGD / ScQGD: QGDCoeffs varScModel7 is not served there")
        var_sc = {"model": model, "ScQGD": opt["ScQGD"], "cSc1": float(md.get("cSc1", 1.0)), "minSc": float(md.get("minSc", -1.0)),
                  "maxSc": float(md.get("maxSc", -1.0)), "const_cells": None}
        if "constScCellSet" in md:     # cells that keep the dictionary's ScQGD [L143-158, L246-254]
            set_name = str(md["constScCellSet"]).strip('"')
            spath = os.path.join(case_dir, "constant", "polyMesh", "sets", set_name)
            if not _exists(spath):
                raise FoamFileError(f"QGD.{model}: constScCellSet '{set_name}': {spath} is missing")
            _, nset, labels = _read_list_file(spath)
            if labels.size != nset:
                raise FoamFileError(f"sets/{set_name}: size mismatch")
            if labels.size and (labels.min() < 0 or labels.max() >= mesh.nCells):
                raise FoamFileError(f"sets/{set_name}: cell label out of range [0, {mesh.nCells})")
            var_sc["const_cells"] = labels.astype(np.int32)
        opt["varSc"] = var_sc          # QGDFoamCase.set_var_sc(**opt["varSc"]); default_options passes it by
    else:
        for k in ("ScQGD", "PrQGD"):   # both default to 1 [constScPrModel1.C L58-89]
            opt[k] = float(md[k]) if k in md else 1.0
    tdir = os.path.join(case_dir, str(time))
    # alphaQGD and ScQGD are READ_IF_PRESENT fields of the time directory [QGDCoeffs.C L119-160, constScPrModel1.C
    # L66-79]: a uniform one becomes the scalar of the options, a non-uniform one travels as (cell values, patch values)
    opt["alphaQGD"] = 0.5
    coeff_fields = {}
    for fname in ("alphaQGD", "ScQGD"):
        fpath = os.path.join(tdir, fname)
        if fname == "ScQGD" and model == "varScModel7":
            continue                   # the model's constructor overwrites the field it reads [varScModel7.C L77-84]: the file is ignored
        if _exists(fpath):
            vals, bvals = read_field(fpath, mesh)
            patch_vals = _patch_values(mesh, vals[:, 0], bvals, fpath)
            if np.all(vals == vals[0]) and np.all(patch_vals == vals[0, 0]):
                opt[fname] = float(vals[0, 0])
            else:
                coeff_fields[fname] = (vals[:, 0].copy(), patch_vals)
    fs_path = os.path.join(case_dir, "system", "fvSchemes")
    fs = read_dict(fs_path)
    # the four fvsc::grad calls [QGDFoam/updateFluxes.H L41-65] and the two qgdFlux calls [L78, L119]
    words, flux = read_face_schemes(fs, ("div(phiJm,U)", "div(phiJm,H)"), ("grad(U)", "grad(e)", "grad(rho)", "grad(p)"), fs_path)
    # the case's `stencil` = the default word when there is one, else grad(U)'s; terms with another word travel as termStencils
    dflt = _find_entry(fs["fvsc"], "default")
    opt["stencil"] = _scheme_words(dflt)[0] if dflt is not None else words["grad(U)"]
    per_term = {t: w for t, w in words.items() if w != opt["stencil"]}
    if len(set(words.values())) > 2:
        raise FoamFileError(f"{fs_path}: fvsc gives the four face gradients more than two distinct stencils ({words}); the resident case "
                            f"serves at most two")
    if per_term:
        opt["termStencils"] = per_term
    opt["fluxSchemeU"] = 1 if flux["div(phiJm,U)"] == "upwind" else 0
    opt["fluxSchemeH"] = 1 if flux["div(phiJm,H)"] == "upwind" else 0
    # (only the implicit branch reads a laplacian scheme: a case whose QGD dictionary has no implicitDiffusion entry runs it, QGDThermo.C L70-82)
    _check_fv_schemes(fs, mesh, need_laplacian=bool(opt["implicitDiffusion"]), need_grad=bool(opt["implicitDiffusion"]), what=fs_path,
                      otherwise="; or the explicit branch, which reads no laplacian scheme: implicitDiffusion false in the QGD dictionary, where the "
                                "entry defaults to true when absent")
    cd = read_dict(os.path.join(case_dir, "system", "controlDict"))
    opt["deltaT"] = float(cd["deltaT"])
    opt["adjustTimeStep"] = 1 if _truthy(cd.get("adjustTimeStep", "no")) else 0
    # createTimeControls.H (L0): maxCo defaults to 1, maxDeltaT to GREAT; setDeltaT-QGDQHD.H L45: cTau defaults to 0.75
    opt["maxCo"] = float(cd.get("maxCo", 1.0))
    opt["maxDeltaT"] = float(cd.get("maxDeltaT", 1e300))
    opt["cTau"] = float(cd.get("cTau", 0.75))

    # the linear solves of the implicitDiffusion branch take fvSolution's controls of U and e [QGDUEqn.H L66, QGDEEqn.H
    # L61: solve(...) looks up solvers.<field>]; the tighter of the two tolerances and the larger maxIter serve both
    # (qgd_case_options has one pair).  OpenFOAM's defaults when an entry is absent: tolerance 1e-6, maxIter 1000.
    if opt["implicitDiffusion"]:
        pairs = [_tol_iter(e) for e in _solver_entries(_fv_solvers(case_dir), ("U", "e", "Ux", "Uy", "Uz"), prefixes=("U.", "e."))]
        if pairs:
            opt["implicitTol"], opt["implicitMaxIter"] = min(t for t, _ in pairs), max(i for _, i in pairs)

    U, bU = read_field(os.path.join(tdir, "U"), mesh)
    T, bT = read_field(os.path.join(tdir, "T"), mesh)
    p, bP = read_field(os.path.join(tdir, "p"), mesh)
    ptw = [PATCH_WORDS.get(int(t), "patch") for t in mesh.array("patchType")]
    bcs = []
    for i, name in enumerate(mesh.patch_names):
        bcs.append({"U": _bc(bU[name], True, ptw[i], f"U.{name}", lists=True), "T": _bc(bT[name], False, ptw[i], f"T.{name}", lists=True),
                    "p": _bc(bP[name], False, ptw[i], f"p.{name}", lists=True)})
    fields = {"U": U, "T": T[:, 0], "p": p[:, 0]}
    fields.update(coeff_fields)
    if species_names:
        opt["species"] = _read_species(case_dir, tdir, tp, species_names, mesh, ptw)   # QGDFoamCase.set_species; default_options passes it by
        if opt["implicitDiffusion"]:
            # YEqn.solve() [QGDYEqn.H L62] looks up solvers.<species name>: the tightest tolerance and the largest maxIter of the transported
            # species serve them all (QGDFoamCase.set_species_solver has one pair)
            solvers = _fv_solvers(case_dir)
            sp = opt["species"]
            pairs = [_solver_controls(solvers, n) for n in sp["names"] if n != sp["inert"]]
            sp["tolerance"], sp["maxIter"] = min(t for t, _ in pairs), max(i for _, i in pairs)
    return mesh, opt, fields, bcs


def _fv_solvers(case_dir):
    """the `solvers` dictionary of system/fvSolution ({} without the file)"""
    path = os.path.join(case_dir, "system", "fvSolution")
    return read_dict(path).get("solvers", {}) if _exists(path) else {}


def _solver_entries(solvers, fields, prefixes=()):
    """the entries of fvSolution.solvers that name one of ``fields``, in the file's order: a key names the words between its quotes,
    parentheses and `|` ("(U|e)" names U and e); with ``prefixes`` also a word that starts with one of them"""
    out = []
    for key, entry in solvers.items() if isinstance(solvers, dict) else ():
        names = str(key).strip('"()').replace("|", " ").split()
        if isinstance(entry, dict) and any(n in fields or n.startswith(tuple(prefixes)) for n in names):
            out.append(entry)
    return out


def _tol_iter(entry):
    """(tolerance, maxIter) of a solver entry; OpenFOAM's defaults 1e-6 and 1000 where it has none"""
    return float(entry.get("tolerance", 1e-6)), int(float(entry.get("maxIter", 1000)))


def _solver_controls(solvers, name):
    """(tolerance, maxIter) of fvSolution.solvers for field `name`: the entry of that name, else the last key that matches it whole as a
    regular expression (OpenFOAM's dictionary lookup; read_dict hands quoted keys over without their quotes, and a plain word matches
    itself only); absent, or an entry without them: OpenFOAM's defaults 1e-6 and 1000"""
    entry = None
    if isinstance(solvers, dict):
        if isinstance(solvers.get(name), dict):
            entry = solvers[name]
        else:
            for key, e in solvers.items():
                try:
                    hit = isinstance(e, dict) and re.fullmatch(str(key), name) is not None
                except re.error:
                    hit = False
                if hit:
                    entry = e
    return _tol_iter(entry or {})


def _species_mixture(tp, names):
    """the one thermo of a case with a `species` list: `mixture{}` where there is one, else the species' own dictionaries, which must all be
    equal -- the composition is passive (no feedback of Y into thermo)"""
    if "mixture" in tp:
        return tp["mixture"]
    dicts = []
    for n in names:
        if not isinstance(tp.get(n), dict):
            raise FoamFileError(f"thermophysicalProperties: neither a mixture dictionary nor one for species '{n}'")
        dicts.append(tp[n])
    for n, d in zip(names[1:], dicts[1:]):
        if d != dicts[0]:
            raise FoamFileError(f"thermophysicalProperties: species '{names[0]}' and '{n}': species with different thermophysical properties are "
                                "not served: the composition is passive")
    return dicts[0]


def _read_species(case_dir, tdir, tp, names, mesh, ptw):
    """the species entries of a reactingLagrangianQGDFoam case: {'names', 'inert', 'ScNumbers' (per species), 'fields' {name: cell values},
    'bcs' {name: per patch (kind, value)}}.  inertSpecie is required and must be a species [createFields.H L31-39]; ScNumbers ((name Sc) ...)
    is optional, names that are no species are ignored, the default is 1 [readScNumbers.H L1-19]; the field of species X is <time>/X, else
    <time>/Ydefault (OpenFOAM's rule); boundary conditions: the patch's own constraint type, zeroGradient, uniform fixedValue."""
    if len(set(names)) != len(names):
        raise FoamFileError(f"thermophysicalProperties: the species list repeats a name: {names}")
    if "inertSpecie" not in tp:
        raise FoamFileError("thermophysicalProperties: a case with species needs inertSpecie [createFields.H L31-39]")
    inert = str(tp["inertSpecie"])
    if inert not in names:
        raise FoamFileError(f"thermophysicalProperties: inertSpecie '{inert}' is not in the species list {names} [createFields.H L31-39]")
    sc = {n: 1.0 for n in names}
    for pair in tp.get("ScNumbers", []) or []:
        if not (isinstance(pair, (list, tuple)) and len(pair) == 2):
            raise FoamFileError(f"thermophysicalProperties: ScNumbers takes (name Sc) pairs, got '{pair}' [readScNumbers.H L1-19]")
        if str(pair[0]) in sc:
            sc[str(pair[0])] = float(pair[1])
    fields, bcs = {}, {}
    for n in names:
        path = os.path.join(tdir, n)
        if not _exists(path):
            path = os.path.join(tdir, "Ydefault")
            if not _exists(path):
                raise FoamFileError(f"{tdir}: neither '{n}' nor 'Ydefault'")
        Y, bY = read_field(path, mesh)
        if Y.shape[1] != 1:
            raise FoamFileError(f"{path}: a species is a volScalarField")
        entries = []
        for i, pn in enumerate(mesh.patch_names):
            kind, val = _bc(bY[pn], False, ptw[i], f"{os.path.basename(path)}.{pn}")
            if kind not in ("none", "zeroGradient", "fixedValue"):
                raise FoamFileError(f"{path}: patch '{pn}': boundary condition '{kind}' of a species is not supported (zeroGradient, uniform fixedValue)")
            entries.append((kind, val))
        fields[n], bcs[n] = Y[:, 0].copy(), entries
    return {"names": names, "inert": inert, "ScNumbers": [sc[n] for n in names], "fields": fields, "bcs": bcs}


def species_entries_text(species):
    """the thermophysicalProperties entries of opt["species"]: what _read_species takes back"""
    pairs = " ".join(f"({n} {_fmt(float(s))})" for n, s in zip(species["names"], species["ScNumbers"]))
    return f"species ({' '.join(species['names'])});\ninertSpecie {species['inert']};\nScNumbers ({pairs});\n"


def apply_species(case, species, cells=None, halo=False):
    """opt["species"] of read_case_setup onto a QGDFoamCase (before set_fields); cells: the case files' labels of the device mesh's cells;
    halo: the device is a shard or serves cyclic patches by ghost copies (QGDFoamCase.set_species halo=True)"""
    # (a case read with implicitDiffusion true carries the species' solver controls: it asks for the implicit branch by name)
    case.set_species(species["names"], species["inert"], ScNumbers=species["ScNumbers"], **({"implicit": True} if species.get("tolerance") is not None else {}),
                     **({"halo": True} if halo else {}))
    if species.get("tolerance") is not None:     # the implicitDiffusion branch: fvSolution.solvers.<species>
        case.set_species_solver(species["tolerance"], species["maxIter"])
    for n in species["names"]:
        for patch, entry in enumerate(species["bcs"][n]):
            case.set_species_bc(n, patch, entry)
        Y = species["fields"][n]
        case.set_species_field(n, Y if cells is None else Y[cells])


def write_species_fields(case_dir, time_name, mesh, species, values):
    """the Y_i files of a time directory: values {name: cell values}; patch entries carry each species' own boundary condition"""
    for n in species["names"]:
        def entry(i, pn, sl):
            kind, val = species["bcs"][n][i]
            return ("fixedValue", np.float64(val)) if kind == "fixedValue" else ("zeroGradient", None)
        write_field(os.path.join(case_dir, str(time_name), n), mesh, n, values[n], _patch_table(mesh, entry))


def _truthy(v):
    return str(v) in ("true", "on", "yes", "1")


def _bc_p_qhd(rec, what):
    """p of a QHDFoam case: zeroGradient | fixedValue (uniform) | fixedGradient (uniform gradient) | qhdFlux.  Inside QHDFoam a
    qhdFlux patch keeps the gradient of its file -- its registry lookup of "phiwStar" finds nothing, the solver registers its flux
    as "phiwo" [qhdFluxFvPatchScalarField.C L166-168] -- so it is read as the fixedGradient patch it behaves like (gradient
    entry, default 0)."""
    t = rec["type"]
    if t in _CONSTRAINT_BCS:
        return ("none", None)
    if t == "zeroGradient":
        return ("zeroGradient", None)
    if t == "fixedValue":
        v = rec["value"]
        if v is None or np.any(v != v[0]):
            raise FoamFileError(f"{what}: fixedValue needs a uniform value")
        return ("fixedValue", float(v[0, 0]))
    if t in ("fixedGradient", "qhdFlux"):
        g = rec.get("gradient")
        if g is None:
            return ("fixedGradient", 0.0)
        g = np.asarray(g, dtype=np.float64).reshape(-1)
        if np.any(g != g[0]):
            raise FoamFileError(f"{what}: only uniform gradients are supported")
        return ("fixedGradient", float(g[0]))
    raise FoamFileError(f"{what}: boundary condition '{t}' is not supported")


def _read_qhd_thermo(case_dir, time, mesh, app):
    """What the QHD family (QHDFoam, SRFQHDFoam, scalarTransportQHDFoam) reads of constant/thermophysicalProperties and <time>/alphaQGD
    alike -> (options, the thermophysicalProperties dictionary): thermoType (equationOfState rhoConst, transport const),
    mixture.equationOfState.rho, mixture.transport.{mu, Pr}, QGD{implicitDiffusion (default true, QGDThermo.C L70-82), QGDCoeffs
    constTau | HbyUQHD | T0byGr | H2bynuQHD with the keys of <model>Dict or of QGD itself [QGDCoeffs.C L81-116; constTau.C L71,
    HbyUQHD.C L61, T0byGr.C L74-75]}; alphaQGD when present and uniform [QGDCoeffs.C L119-160, default 0.5].  ``app`` names the
    application in the refusals."""
    opt = {}
    tp = read_dict(os.path.join(case_dir, "constant", "thermophysicalProperties"))
    tt = tp.get("thermoType", {})
    for key, want in (("equationOfState", "rhoConst"), ("transport", "const")):
        if isinstance(tt, dict) and key in tt and str(tt[key]) != want:
            raise FoamFileError(f"thermoType.{key} '{tt[key]}' is not supported by the {app} path (only {want})")
    mix = tp["mixture"]
    opt["rho0"] = float(mix["equationOfState"]["rho"])
    opt["mu"], opt["Pr"] = float(mix["transport"]["mu"]), float(mix["transport"]["Pr"])
    qgd = tp["QGD"]
    opt["implicitDiffusion"] = 1 if _truthy(qgd.get("implicitDiffusion", "true")) else 0
    model = str(qgd["QGDCoeffs"])
    if model not in ("constTau", "HbyUQHD", "T0byGr", "H2bynuQHD"):
        raise FoamFileError(f"QGDCoeffs '{model}' is not a closure of the {app} path (constTau, HbyUQHD, T0byGr, H2bynuQHD)")
    opt["tauModel"] = model
    md = qgd.get(model + "Dict", qgd)
    for key, needed in (("Tau", model == "constTau"), ("UQHD", model == "HbyUQHD"), ("T0", model == "T0byGr"), ("Gr", model == "T0byGr")):
        if needed:
            if key not in md:
                raise FoamFileError(f"QGD.{model}: entry '{key}' is missing")
            opt[key] = float(md[key])
    opt["aQGD"] = 0.5
    apath = os.path.join(case_dir, str(time), "alphaQGD")
    if _exists(apath):
        vals, _ = read_field(apath, mesh)
        if not np.all(vals == vals[0]):
            raise FoamFileError(f"{apath}: a non-uniform alphaQGD is not supported by the {app} path")
        opt["aQGD"] = float(vals[0, 0])
    return opt, tp


def _qhd_patch_bcs(mesh, bU, bT, app, velocity="U", velocity_bc=None, bP=None):
    """per patch {'U': ..., 'T': ...[, 'p': ...]} of a QHD-family case from the patch records of its velocity, T and (QHDFoam) p files;
    qgdFlux, and slip on T, are refused"""
    ptw = [PATCH_WORDS.get(int(t), "patch") for t in mesh.array("patchType")]
    bcs = []
    for i, name in enumerate(mesh.patch_names):
        bu = (velocity_bc or _bc)(bU[name], True, ptw[i], f"{velocity}.{name}")
        bt = _bc(bT[name], False, ptw[i], f"T.{name}")
        if bu[0] == "qgdFlux" or bt[0] in ("qgdFlux", "slip"):
            raise FoamFileError(f"patch {name}: boundary condition not supported for {velocity} / T of a {app} case")
        bcs.append({"U": bu, "T": bt} if bP is None else {"U": bu, "T": bt, "p": _bc_p_qhd(bP[name], f"p.{name}")})
    return bcs


def read_run_control(cd):
    """the run control of system/controlDict: {endTime, writeInterval, writeControl, timePrecision} with OpenFOAM's defaults"""
    return {"endTime": float(cd["endTime"]), "writeInterval": float(cd.get("writeInterval", 1)),
            "writeControl": str(cd.get("writeControl", "timeStep")), "timePrecision": int(cd.get("timePrecision", 6))}


def read_qhd_case_setup(case_dir, time="0", velocity="U", velocity_bc=None, time_control=False):
    """Read an OpenFOAM QHDFoam case directory [QHDFoam.C L63-72, QHDFoam/createFields.H L32-167].
    (velocity / velocity_bc: the name of the velocity file and the reading of its patch entries, for read_srf_case_setup.)

    Returns (mesh, options dict for ``qhdfoam.qhd_options``, {'U','T','p'} internal arrays, per-patch BC triples) and, with
    ``time_control``, a fifth item: {adjustTimeStep, maxCo, maxDeltaT, cTau} of system/controlDict [readTimeControls.H;
    setDeltaT-QGDQHD.H L45] with the defaults no, 1, GREAT, 0.75 -- for ``QHDFoamCase.set_time_control``.  Without ``time_control`` the
    caller drives a fixed deltaT, and ``adjustTimeStep yes`` is refused.
    Entries read: constant/polyMesh; constant/thermophysicalProperties -- thermoType (equationOfState rhoConst, transport const),
    mixture.equationOfState.rho, mixture.transport.{mu, Pr, beta} [createFields.H L110-115], QGD{implicitDiffusion (default true,
    QGDThermo.C L70-82), QGDCoeffs constTau | HbyUQHD | T0byGr | H2bynuQHD with the keys of <model>Dict or of QGD itself
    [QGDCoeffs.C L81-116; constTau.C L71, HbyUQHD.C L61, T0byGr.C L74-75], pRefCell, pRefValue [createFields.H L162-165]};
    constant/gravitationalProperties g [createFields.H L96-108]; <time>/alphaQGD when present and uniform [QGDCoeffs.C L119-160,
    default 0.5]; system/fvSchemes fvsc.default; system/controlDict deltaT; system/fvSolution solvers.p {tolerance, relTol,
    maxIter} and, with implicitDiffusion, solvers.(U|T) {tolerance, maxIter}; <time>/{U,T,p}."""
    mesh = read_polymesh(os.path.join(case_dir, "constant", "polyMesh"))
    _refuse_unserved_patches(mesh, case_dir)
    opt, tp = _read_qhd_thermo(case_dir, time, mesh, "QHDFoam")
    opt["beta"] = float(tp["mixture"]["transport"]["beta"])
    qgd = tp["QGD"]
    opt["pRefCell"] = int(float(qgd.get("pRefCell", 0)))      # setRefCell(p, thermo.subDict("QGD"), ...) [createFields.H L165]
    opt["pRefValue"] = float(qgd.get("pRefValue", 0.0))
    gp = read_dict(os.path.join(case_dir, "constant", "gravitationalProperties"))
    g = gp["g"]
    g = [x for x in (g if isinstance(g, (list, tuple, np.ndarray)) else [g])]
    # `g g [0 1 -2 0 0 0 0] (0 -9.81 0);`, `g [0 1 -2 0 0 0 0] (0 -9.81 0);` or `g (0 -9.81 0);`: the vector is the last list of 3
    vec = None
    for item in reversed(g):
        if isinstance(item, (list, tuple, np.ndarray)) and len(item) == 3:
            vec = [float(x) for x in item]
            break
    if vec is None and len(g) == 3 and all(isinstance(x, (int, float)) for x in g):
        vec = [float(x) for x in g]
    if vec is None:
        raise FoamFileError(f"{case_dir}/constant/gravitationalProperties: cannot read the vector g")
    opt["g"] = tuple(vec)
    tdir = os.path.join(case_dir, str(time))
    fs_path = os.path.join(case_dir, "system", "fvSchemes")
    fs = read_dict(fs_path)
    # fvsc::grad of U, W, T [QHDFoam/updateFields.H L36-40] and p [QHDUEqn.H L36]; qgdFlux(phi,U,Uf) [QHDUEqn.H L41], qgdFlux(phi,T,Tf) [QHDTEqn.H L65]
    words, flux = read_face_schemes(fs, ("div(phi,U)", "div(phi,T)"), ("grad(U)", "grad(W)", "grad(T)", "grad(p)"), fs_path)
    used = {t: w for t, w in words.items() if t != "grad(W)"}     # gradWf [QHDFoam/updateFields.H L38] is formed by the reference and never consumed
    if len(set(used.values())) > 1:
        raise FoamFileError(f"{fs_path}: fvsc gives different stencils to different terms ({used}); the resident QHDFoam case runs ONE stencil "
                            f"for its face gradients -- use the fvsc operators of a Device for mixed stencils")
    opt["stencil"] = used["grad(U)"]
    opt["fluxSchemeU"] = 1 if flux["div(phi,U)"] == "upwind" else 0
    opt["fluxSchemeT"] = 1 if flux["div(phi,T)"] == "upwind" else 0
    _check_fv_schemes(fs, mesh, need_laplacian=True, need_grad=True, what=fs_path)
    cd = read_dict(os.path.join(case_dir, "system", "controlDict"))
    opt["deltaT"] = float(cd["deltaT"])
    adjust = _truthy(cd.get("adjustTimeStep", "no"))
    if adjust and not time_control:
        raise FoamFileError("adjustTimeStep yes: the QHDFoam path runs with the fixed deltaT of controlDict (its matrices are built once) "
                            "unless the caller asks for the time controls (time_control=True) and hands them to QHDFoamCase.set_time_control")
    # runTime.controlDict().lookupOrDefault [readTimeControls.H, L0]: maxCo 1, maxDeltaT GREAT; cTau 0.75 [setDeltaT-QGDQHD.H L45]
    tc = {"adjustTimeStep": bool(adjust), "maxCo": float(cd.get("maxCo", 1.0)), "maxDeltaT": float(cd.get("maxDeltaT", 1e300)),
          "cTau": float(cd.get("cTau", 0.75))}
    solvers = _fv_solvers(case_dir)
    for entry in _solver_entries(solvers, ("p",)):      # (the last entry that names p wins, key by key)
        opt["pTol"], opt["pMaxIter"] = _tol_iter(entry)
        opt["pRelTol"] = float(entry.get("relTol", 0.0))
    pairs = [_tol_iter(e) for e in _solver_entries(solvers, ("U", "T", "Ux", "Uy", "Uz"))]
    if pairs and opt["implicitDiffusion"]:
        opt["implicitTol"], opt["implicitMaxIter"] = min(t for t, _ in pairs), max(i for _, i in pairs)
    if not _exists(os.path.join(tdir, velocity)):
        raise FoamFileError(f"{tdir}: the velocity file '{velocity}' is missing")
    U, bU = read_field(os.path.join(tdir, velocity), mesh)
    T, bT = read_field(os.path.join(tdir, "T"), mesh)
    p, bP = read_field(os.path.join(tdir, "p"), mesh)
    bcs = _qhd_patch_bcs(mesh, bU, bT, "QHDFoam", velocity, velocity_bc, bP)
    out = (mesh, opt, {"U": U, "T": T[:, 0], "p": p[:, 0]}, bcs)
    return out + (tc,) if time_control else out


def read_scalar_case_setup(case_dir, time="0"):
    """Read an OpenFOAM scalarTransportQHDFoam case directory [scalarTransportQHDFoam.C L60-84, its createFields.H].

    Returns (mesh, options dict for ``scalarfoam.scalar_options``, {'U','T'} internal arrays, per-patch BC pairs, run control dict
    {endTime, writeInterval}).  Entries read: constant/polyMesh; constant/thermophysicalProperties -- thermoType (equationOfState
    rhoConst, transport const), mixture.equationOfState.rho, mixture.transport.{mu, Pr}, QGD{implicitDiffusion (default true,
    QGDThermo.C L70-82), QGDCoeffs constTau | HbyUQHD | T0byGr | H2bynuQHD with the keys of <model>Dict or of QGD itself}; <time>/alphaQGD
    when present and uniform; system/fvSchemes fvsc (grad(T), else default), divSchemes `div(phiu,T)`, interpolationSchemes, ddt /
    laplacian schemes; system/controlDict deltaT, endTime, writeInterval, adjustTimeStep, maxCo, maxDeltaT, cTau (default 0.75,
    setDeltaT-QGDQHD.H L48); system/fvSolution solvers.T {tolerance, maxIter}; <time>/{U,T}.  What the path would compute differently
    is refused by name."""
    mesh = read_polymesh(os.path.join(case_dir, "constant", "polyMesh"))
    _refuse_unserved_patches(mesh, case_dir)
    opt, _ = _read_qhd_thermo(case_dir, time, mesh, "scalarTransportQHDFoam")
    tdir = os.path.join(case_dir, str(time))
    fs_path = os.path.join(case_dir, "system", "fvSchemes")
    fs = read_dict(fs_path)
    words, flux = read_face_schemes(fs, ("div(phiu,T)",), ("grad(T)",), fs_path)   # fvsc::grad(T) [updateFields.H L1], qgdFlux(phiu,T,Tf) [.C L110]
    opt["stencil"] = words["grad(T)"]
    opt["fluxSchemeT"] = 1 if flux["div(phiu,T)"] == "upwind" else 0
    _check_fv_schemes(fs, mesh, need_laplacian=True, need_grad=False, what=fs_path)
    cd = read_dict(os.path.join(case_dir, "system", "controlDict"))
    opt["deltaT"] = float(cd["deltaT"])
    opt["adjustTimeStep"] = 1 if _truthy(cd.get("adjustTimeStep", "no")) else 0
    if opt["adjustTimeStep"]:
        opt["maxCo"] = float(cd.get("maxCo", 1.0))                 # runTime.controlDict().lookupOrDefault [readTimeControls.H, L0]
        opt["maxDeltaT"] = float(cd.get("maxDeltaT", 1e300))       # GREAT
        opt["cTau"] = float(cd.get("cTau", 0.75))
    control = read_run_control(cd)
    for entry in _solver_entries(_fv_solvers(case_dir), ("T",)):      # (the last entry that names T wins)
        opt["implicitTol"], opt["implicitMaxIter"] = _tol_iter(entry)
    U, bU = read_field(os.path.join(tdir, "U"), mesh)
    T, bT = read_field(os.path.join(tdir, "T"), mesh)
    bcs = _qhd_patch_bcs(mesh, bU, bT, "scalarTransportQHDFoam")
    return mesh, opt, {"U": U, "T": T[:, 0]}, bcs, control


def assemble_scalar_case(mesh, opt, fields, bcs, device_id=0):
    """what read_scalar_case_setup returned -> (Device, ScalarTransportQHDCase) ready to ``step()``"""
    from .fvsc import Device
    from .scalarfoam import ScalarTransportQHDCase, scalar_options

    dev = Device(mesh, device_id, fv_schemes={"fvsc": {"default": opt["stencil"]}}, fused_tables=False)
    case = ScalarTransportQHDCase(dev, scalar_options(**opt))
    for i, bc in enumerate(bcs):
        case.set_bc(i, U=bc["U"], T=bc["T"])
    case.set_fields(fields["U"], fields["T"])
    return dev, case


def load_scalar_case(case_dir, time="0", device_id=0):
    """Case directory -> (Device, ScalarTransportQHDCase) ready to ``step()``"""
    return assemble_scalar_case(*read_scalar_case_setup(case_dir, time)[:4], device_id)


def write_scalar_time(case, case_dir, time_name, U, bcs=None, rho0=None):
    """T of a ScalarTransportQHDCase, the frozen U it was started with and the uniform rho into <case_dir>/<time_name>/ (the AUTO_WRITE
    fields of scalarTransportQHDFoam); T's patch entries carry the patch values as ``value``"""
    mesh = case.mesh
    Tb = case.field("T.boundary")
    rho = float(rho0 if rho0 is not None else case.options.rho0)

    def entry_T(i, pn, sl):
        kT = bcs[i]["T"][0] if bcs is not None else "calculated"
        return ("calculated" if kT == "none" else kT, Tb[sl])

    def entry_U(i, pn, sl):
        kU, vU = bcs[i]["U"] if bcs is not None else ("zeroGradient", None)
        return (kU, np.asarray(vU, dtype=np.float64)) if kU == "fixedValue" else (kU, None)

    d = os.path.join(case_dir, str(time_name))
    write_field(os.path.join(d, "T"), mesh, "T", case.field("T"), _patch_table(mesh, entry_T), _DIMS["T"])
    write_field(os.path.join(d, "U"), mesh, "U", np.asarray(U, dtype=np.float64).reshape(-1, 3), _patch_table(mesh, entry_U), _DIMS["U"])
    write_field(os.path.join(d, "rho"), mesh, "rho", np.full(mesh.nCells, rho), _patch_table(mesh, lambda i, pn, sl: ("calculated", np.float64(rho))),
                _DIMS["rho"])


def assemble_qhd_case(mesh, opt, fields, bcs, device_id=0, fused_tables=True, omega=None, solve_T=False):
    """what read_qhd_case_setup / read_srf_case_setup returned -> (Device, QHDFoamCase) ready to ``step()``: the createFields.H sequence
    of QHDFoam -- with ``omega``, of SRFQHDFoam: the case in the rotating frame -- over the C-ABI.  A velocity given per face
    (read_srf_case_setup) goes through set_bc_values, after the patch's entry."""
    from .fvsc import Device
    from .qhdfoam import QHDFoamCase, qhd_options

    dev = Device(mesh, device_id, fv_schemes={"fvsc": {"default": opt["stencil"]}}, fused_tables=fused_tables)
    case = QHDFoamCase(dev, qhd_options(**opt))
    if omega is not None:
        case.set_srf(omega, solve_T=solve_T)
    apply_qhd_bcs(case, bcs)
    case.set_fields(fields["U"], fields["T"], fields["p"])
    return dev, case


def load_qhd_case(case_dir, time="0", device_id=0):
    """Case directory -> (Device, QHDFoamCase) ready to ``step()``: the createFields.H sequence of QHDFoam over the C-ABI."""
    return assemble_qhd_case(*read_qhd_case_setup(case_dir, time), device_id)


def read_srf_case_setup(case_dir, time="0", time_control=False):
    """Read an OpenFOAM SRFQHDFoam case directory [SRFQHDFoam.C L70-81, SRFQHDFoam/createFields.H L22-39]: what read_qhd_case_setup reads,
    with the relative velocity ``Urel`` in place of ``U``, and constant/SRFProperties.

    Returns (mesh, options dict, {'U' (= Urel),'T','p'}, per-patch BC triples, srf) with srf = {'omega', 'origin', 'axis', 'rpm'} and,
    with ``time_control``, the time controls of read_qhd_case_setup as a sixth item (without it ``adjustTimeStep yes`` is refused).
    SRFProperties: ``SRFModel rpm; origin (x y z); axis (x y z); rpmCoeffs { rpm N; }`` and omega = axis/|axis| * rpm * 2 pi / 60.
    ASSUMPTION (L0): a restatement of OpenFOAM v2312's SRF::SRFModel (origin, axis normalised on reading) and SRF::rpm
    (omega = axis * rpm * twoPi / 60); their sources are not among the reference's listings.
    Patch entries of Urel: what QHDFoam's U takes, a fixedValue entry also as a value list, and ``SRFVelocity`` (OpenFOAM v2312
    SRFVelocityFvPatchVectorField::updateCoeffs, L0): ``relative yes`` is fixedValue inletValue; ``relative no`` (a wall at rest in the
    inertial frame) is one value per face, inletValue - omega ^ (Cf - origin), returned as an (nFaces, 3) array for
    QHDFoamCase.set_bc_values.  Refused by name: any other SRFModel, SRFFreestreamVelocity, a missing Urel, a non-uniform inletValue."""
    sp_path = os.path.join(case_dir, "constant", "SRFProperties")
    if not _exists(sp_path):
        raise FoamFileError(f"{sp_path}: SRFQHDFoam needs constant/SRFProperties")
    sp = read_dict(sp_path)
    model = str(sp.get("SRFModel", ""))
    if model != "rpm":
        raise FoamFileError(f"{sp_path}: SRFModel '{model}' is not supported (only rpm)")

    def vec(key):
        try:
            v = np.asarray(sp[key], dtype=np.float64).reshape(-1)
        except (KeyError, TypeError, ValueError):
            v = np.zeros(0)
        if v.size != 3 or not np.isfinite(v).all():
            raise FoamFileError(f"{sp_path}: entry '{key}' must be a vector")
        return v

    origin, axis = vec("origin"), vec("axis")
    if not np.linalg.norm(axis) > 0:
        raise FoamFileError(f"{sp_path}: axis must not vanish")
    coeffs = sp.get("rpmCoeffs", sp)
    if not isinstance(coeffs, dict) or "rpm" not in coeffs:
        raise FoamFileError(f"{sp_path}: rpmCoeffs.rpm is missing")
    rpm = float(coeffs["rpm"])
    omega = axis / np.linalg.norm(axis) * (rpm * 2.0 * np.pi / 60.0)
    tdir = os.path.join(case_dir, str(time))
    if not _exists(os.path.join(tdir, "Urel")):
        raise FoamFileError(f"{tdir}: SRFQHDFoam reads the relative velocity from the file Urel [SRFQHDFoam/createFields.H L22-33]; there is none"
                            + (" (the directory has a file U: rename it, and give the walls at rest the type SRFVelocity)"
                               if _exists(os.path.join(tdir, "U")) else ""))
    # (the patch geometry before the fields: the reading of a `relative no` entry needs the face centres)
    geo = read_polymesh(os.path.join(case_dir, "constant", "polyMesh"))
    names, Cf = list(geo.patch_names), geo.array("Cf").reshape(-1, 3)
    start, size = [int(x) for x in geo.array("patchStart")], [int(x) for x in geo.array("patchSize")]

    def urel_bc(rec, vector, patch_type_word, what):
        t = rec["type"]
        if t == "SRFFreestreamVelocity":
            raise FoamFileError(f"{what}: boundary condition 'SRFFreestreamVelocity' is not supported")
        if t != "SRFVelocity":
            return _bc(rec, vector, patch_type_word, what, lists=True)
        if patch_type_word in _CONSTRAINT_BCS:
            raise FoamFileError(f"{what}: inconsistent patch and patchField types: the patch is '{patch_type_word}', the field says '{t}'")
        if "inletValue" not in rec or "relative" not in rec:
            raise FoamFileError(f"{what}: SRFVelocity needs the entries relative and inletValue")
        iv = rec["inletValue"]
        if not (isinstance(iv, list) and len(iv) == 2 and iv[0] == "uniform"):
            raise FoamFileError(f"{what}: only a uniform inletValue is supported")
        iv = np.asarray(iv[1], dtype=np.float64).reshape(-1)
        if iv.size != 3:
            raise FoamFileError(f"{what}: inletValue must be a vector")
        if _truthy(rec["relative"]):
            return ("fixedValue", iv)
        i = names.index(what.split(".", 1)[1])
        return ("fixedValue", iv[None, :] - np.cross(omega, Cf[start[i]: start[i] + size[i]] - origin))

    mesh, opt, fields, bcs, *tc = read_qhd_case_setup(case_dir, time, velocity="Urel", velocity_bc=urel_bc, time_control=time_control)
    return (mesh, opt, fields, bcs, dict(omega=omega, origin=origin, axis=axis / np.linalg.norm(axis), rpm=rpm)) + tuple(tc)


def apply_qhd_bcs(case, bcs):
    """the per-patch triples of read_qhd_case_setup / read_srf_case_setup onto a QHDFoamCase: a velocity given per face goes through
    set_bc_values, after the patch's entry"""
    for i, bc in enumerate(bcs):
        u = bc["U"]
        per_face = u[0] == "fixedValue" and np.ndim(u[1]) == 2
        case.set_bc(i, U=("fixedValue", (0.0, 0.0, 0.0)) if per_face else u, T=bc["T"], p=bc["p"])
        if per_face:
            case.set_bc_values(i, u[1])


def load_srf_case(case_dir, time="0", device_id=0, solve_T=False):
    """Case directory -> (Device, QHDFoamCase in the rotating frame, srf) ready to ``step()``: SRFQHDFoam's createFields.H over the C-ABI"""
    mesh, opt, fields, bcs, srf = read_srf_case_setup(case_dir, time)
    return assemble_qhd_case(mesh, opt, fields, bcs, device_id, omega=srf["omega"], solve_T=solve_T) + (srf,)


def write_srf_time(case, case_dir, time_name, srf, bcs=None):
    """Urel, p, T (as read, unless the case solves it) and Uabs = Urel + omega ^ (C - origin) of a rotating QHDFoamCase into
    <case_dir>/<time_name>/.  A patch whose velocity is given per face (SRFVelocity with `relative no`) is written as the fixedValue
    list it evaluates to, which read_srf_case_setup reads back bit for bit; Uabs carries calculated patch values."""
    mesh = case.mesh
    write_qhd_time(case, case_dir, time_name, bcs, velocity="Urel")
    omega, origin = np.asarray(srf["omega"], dtype=np.float64), np.asarray(srf["origin"], dtype=np.float64)
    Uabs = case.field("U") + np.cross(omega, mesh.array("C").reshape(-1, 3) - origin)
    Ub = case.field("U.boundary") + np.cross(omega, mesh.array("Cf").reshape(-1, 3)[mesh.nInternalFaces:] - origin)
    write_field(os.path.join(case_dir, str(time_name), "Uabs"), mesh, "Uabs", Uabs, _patch_table(mesh, lambda i, pn, sl: ("calculated", Ub[sl])),
                _DIMS["U"])


def write_qhd_time(case, case_dir, time_name, bcs=None, velocity="U"):
    """U, T, p of a QHDFoamCase into <case_dir>/<time_name>/ (the AUTO_WRITE fields of QHDFoam that this path carries); patch
    entries carry the patch values as ``value`` (fixedGradient patches also their ``gradient``).  velocity: the name of U's file."""
    mesh = case.mesh
    if hasattr(mesh, "file_mesh"):
        raise FoamFileError("write_time: a case with cyclic patches carries copies of its cells; python -m qgdsolver_amd.QGDFoam writes its time directories")
    for fname in ("U", "T", "p"):
        bvals = case.field(fname + ".boundary")

        def entry(i, pn, sl):
            kind = _written_kind(bcs, i, fname)
            if kind == "fixedGradient":
                return (kind, bvals[sl], {"gradient": float(bcs[i][fname][1] or 0.0)})
            return (kind, bvals[sl])
        out_name = velocity if fname == "U" else fname
        write_field(os.path.join(case_dir, str(time_name), out_name), mesh, out_name, case.field(fname), _patch_table(mesh, entry), _QHD_DIMS[fname])


def _patch_values(mesh, internal, patches, what):
    """patch values (nBoundaryFaces) of a scalar field read by read_field: `value` where the file gives one, otherwise
    the owner cell's value (zeroGradient / calculated without value; also on constraint patches, which carry no field)"""
    nif = mesh.nInternalFaces
    own = mesh.array("owner")
    out = np.zeros(mesh.nBoundaryFaces)
    ps, pz, pt = mesh.array("patchStart"), mesh.array("patchSize"), mesh.array("patchType")
    names = getattr(mesh, "patch_names", None) or [f"patch{i}" for i in range(mesh.nPatches)]
    for i, name in enumerate(names):
        sl = slice(int(ps[i]) - nif, int(ps[i]) - nif + int(pz[i]))
        if PATCH_WORDS.get(int(pt[i]), "patch") in _CONSTRAINT_BCS:
            out[sl] = internal[own[int(ps[i]): int(ps[i]) + int(pz[i])]]   # carries no field; never read
            continue
        rec = patches[name]
        if rec["value"] is not None:
            out[sl] = rec["value"][:, 0]
        elif rec["type"] in ("zeroGradient", "calculated"):
            out[sl] = internal[own[int(ps[i]): int(ps[i]) + int(pz[i])]]
        else:
            raise FoamFileError(f"{what}: patch '{name}' of type '{rec['type']}' needs a value")
    return out


def _is_value_list(field, value):
    """whether a fixedValue entry's value is one value per face ((nFaces, 3) for U, (nFaces,) for T and p) and not the patch's one value"""
    return value is not None and np.ndim(value) == (2 if field == "U" else 1)


def device_bcs(file_mesh, mesh, bcs):
    """the per-patch BC triples of the case files for a device mesh cut or unrolled from file_mesh: value lists of fixedValue entries follow
    the device mesh's patch faces.  A shard's patch faces (those of its ghost cells included) are found through faceGlobal; on a mesh from
    unroll_cyclic the real faces keep their order and a copy's face (faceGlobal = -1 - label) takes the value of the face it copies -- its
    record is its original's anyway (the library refreshes it), the entry only serves the start-up evaluation."""
    if mesh is file_mesh or not any(_is_value_list(f, bc[f][1]) for bc in bcs for f in ("U", "T", "p") if bc[f][0] == "fixedValue"):
        return bcs
    fg = mesh.array("faceGlobal")
    ps, pz = mesh.array("patchStart"), mesh.array("patchSize")
    gps, gpz = file_mesh.array("patchStart"), file_mesh.array("patchSize")
    out = []
    for i, bc in enumerate(bcs):
        rec = dict(bc)
        for f in ("U", "T", "p"):
            kind, val = bc[f]
            if kind == "fixedValue" and _is_value_list(f, val):
                g = fg[int(ps[i]): int(ps[i]) + int(pz[i])].astype(np.int64)
                g = np.where(g < 0, -1 - g, g) - int(gps[i])
                if g.size and (g.min() < 0 or g.max() >= int(gpz[i])):
                    raise FoamFileError(f"patch {i}: a face of the device mesh does not belong to the same patch of the case's mesh")
                rec[f] = (kind, np.asarray(val, dtype=np.float64)[g])
        out.append(rec)
    return out


def apply_bcs(case, file_mesh, mesh, bcs):
    """the per-patch BC triples of read_case_setup onto a QGDFoamCase on ``mesh`` (file_mesh itself, or cut or unrolled from it: device_bcs)"""
    for i, bc in enumerate(device_bcs(file_mesh, mesh, bcs)):
        case.set_bc(i, U=bc["U"], T=bc["T"], p=bc["p"])


def load_case(case_dir, time="0", device_id=0):
    """Case directory -> (Device, QGDFoamCase) ready to ``step()``: the createFields.H sequence of QGDFoam over the
    C-ABI.  Needs the HIP device (there is no CPU fallback)."""
    from .fvsc import Device
    from .qgdfoam import QGDFoamCase, default_options

    file_mesh, opt, fields, bcs = read_case_setup(case_dir, time)
    mesh = file_mesh
    if getattr(file_mesh, "cyclic_pairs", None):
        # translational cyclic pairs: glued, with translated copies of the cells behind either half (PolyMesh.unroll_cyclic); the real cells
        # keep their labels, case.field(...)[:case.mesh.file_mesh.nCells] are theirs
        if opt.get("implicitDiffusion") or "alphaQGD" in fields or "ScQGD" in fields:
            raise FoamFileError(f"{case_dir}: a case with cyclic patches runs the explicit branch (QGD {{ implicitDiffusion false; }}) with uniform alphaQGD / ScQGD")
        mesh = file_mesh.unroll_cyclic(file_mesh.cyclic_pairs)
        mesh.file_mesh = file_mesh
        cg = mesh.array("cellGlobal")
        fields = {k: v[cg] for k, v in fields.items()}
    dev = Device(mesh, device_id, fv_schemes={"fvsc": {"default": opt["stencil"]}})
    case = QGDFoamCase(dev, default_options(**opt))
    apply_bcs(case, file_mesh, mesh, bcs)
    if "alphaQGD" in fields or "ScQGD" in fields:
        case.set_qgd_coeffs(alphaQGD=fields.get("alphaQGD"), ScQGD=fields.get("ScQGD"))
    if opt.get("varSc"):
        case.set_var_sc(**opt["varSc"])
    if opt.get("species"):
        # (cyclic patches: the copies behind either half carry their originals' composition, which the library refreshes with their records)
        cyclic = hasattr(mesh, "file_mesh")
        apply_species(case, opt["species"], *((mesh.array("cellGlobal"), True) if cyclic else ()))
    case.set_fields(fields["U"], fields["T"], fields["p"])
    return dev, case


def write_time(case, case_dir, time_name, bcs=None, species=None):
    """Write U, T, p, rho of a QGDFoamCase -- and, with ``species`` (opt["species"] of read_case_setup), every Y_i -- into <case_dir>/<time_name>/ (what runTime.write() leaves for QGDFoam's
    AUTO_WRITE fields); patch entries carry the patch values as ``value`` -- a fixedValue entry what the case prescribes there
    (``uniform`` for one value per patch, ``nonuniform List<...>`` for a value list: what the reader takes back), zeroGradient / slip /
    qgdFlux entries none (the case evaluates them at start-up; the reader refuses a value list there)."""
    mesh = case.mesh
    if hasattr(mesh, "file_mesh"):
        raise FoamFileError("write_time: a case with cyclic patches carries copies of its cells; python -m qgdsolver_amd.QGDFoam writes its time directories")
    for fname in ("U", "T", "p", "rho"):
        bvals = case.field(fname + ".boundary")

        def entry(i, pn, sl):
            kind = _written_kind(bcs, i, fname)
            if kind == "fixedValue" and fname != "rho":
                vals, is_list = case.get_bc_values(i, fname)
                return (kind, vals if is_list or not len(vals) else vals[0])
            return (kind, None) if kind in ("zeroGradient", "slip", "qgdFlux") else (kind, bvals[sl])
        write_field(os.path.join(case_dir, str(time_name), fname), mesh, fname, case.field(fname), _patch_table(mesh, entry), _DIMS[fname])
    if species:
        write_species_fields(case_dir, time_name, mesh, species, {n: case.species_field(n) for n in species["names"]})


def write_cell_fields(case_dir, name, data, bcs, file_mesh, var_sc=None):
    """Time directory from gathered cell fields (the QGDFoam application: write_time's job for a run whose cells are relabelled, cut into
    shards or carry cyclic copies).  Patch entries carry the BC type; values of fixedValue patches are
    the prescribed ones, the others are written without a value (the solver evaluates them at start-up).  ScQGD (varScModel7) has
    calculated patches with the dictionary's value, clipped like the field [varScModel7.C L237-244]."""
    sc_b = None
    if var_sc:
        sc_b = var_sc["ScQGD"]
        sc_b = max(sc_b, var_sc["minSc"]) if var_sc["minSc"] >= 0 else sc_b
        sc_b = min(sc_b, var_sc["maxSc"]) if var_sc["maxSc"] >= 0 else sc_b
    for fname, values in data.items():
        def entry(i, pn, sl):
            if fname == "ScQGD":
                return ("calculated", np.float64(sc_b))
            kind, val = bcs[i].get(fname, ("calculated", None)) if fname != "rho" else ("calculated", None)
            return ("calculated" if kind == "none" else kind, np.asarray(val, dtype=np.float64) if (kind == "fixedValue" and val is not None) else None)
        write_field(os.path.join(case_dir, str(name), fname), file_mesh, fname, values, _patch_table(file_mesh, entry), _DIMS[fname])
