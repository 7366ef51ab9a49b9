"""CPU: the Python mirror of QGD_SPECIES_HALO -- foamfile.apply_species asks for it only when told to, QGDFoamCase.set_species(halo=True)
sets bit 4 of the flags of qgd_case_set_species."""
import ctypes as C

import numpy as np

from qgdsolver_amd import _lib as L
from qgdsolver_amd import foamfile as ff
from qgdsolver_amd.qgdfoam import QGDFoamCase

from test_species_implicit_reader import RecordingCase
from test_species_reader import write_species_case


def test_apply_species_passes_halo_only_when_asked(tmp_path):
    write_species_case(tmp_path)
    species = ff.read_case_setup(str(tmp_path))[1]["species"]
    cells = np.arange(species["fields"]["N2"].size)[::-1].copy()
    for args, kw, want in (((), {}, None), ((cells,), {}, None), ((cells,), {"halo": False}, None), ((cells,), {"halo": True}, True),
                           ((None, True), {}, True)):
        case = RecordingCase()
        ff.apply_species(case, species, *args, **kw)
        name, a, k = case.calls[0]
        assert name == "set_species" and a == (species["names"], species["inert"]) and k.get("halo") is want and ("halo" in k) == bool(want), (args, kw, k)
        assert "implicit" not in k
        fields = [c for c in case.calls if c[0] == "set_species_field"]
        assert len(fields) == 3 and all(np.array_equal(c[1][1], species["fields"][c[1][0]][cells] if args and args[0] is not None else species["fields"][c[1][0]]) for c in fields)


class FakeLib:
    def __init__(self):
        self.flags = []

    def qgd_case_set_species(self, h, n, inert, sc, flags):
        self.flags.append(int(flags))
        return 0


def test_set_species_sets_bit_4(monkeypatch):
    assert (L.SPECIES_KEEP_FLUXES, L.SPECIES_IMPLICIT, L.SPECIES_HALO) == (1, 2, 4)
    header = open(ff.os.path.join(ff.os.path.dirname(ff.os.path.dirname(ff.os.path.abspath(ff.__file__))), "include", "qgd_amd.h")).read()
    assert "#define QGD_SPECIES_HALO 4" in header and "#define QGD_ABI_VERSION 9" in header
    fake = FakeLib()
    monkeypatch.setattr(L, "lib", fake)
    case = object.__new__(QGDFoamCase)
    case._handle = C.c_void_p(0)
    case.set_species(["A", "B"], "B")
    case.set_species(["A", "B"], "B", halo=True)
    case.set_species(["A", "B"], "B", keep_fluxes=True, implicit=True, halo=True)
    case.set_species(["A", "B"], "B", keep_fluxes=True, implicit=True)
    assert fake.flags == [0, 4, 7, 3]
