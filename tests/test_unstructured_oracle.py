"""The CPU restatement for unstructured 2-D quadrilateral meshes (tests/unstructured_oracle.py) reproduces the reference's own
numbers on its two such meshes (tests/golden/reference_kat_unstructured.json).  No GPU, no library: numpy only.

  * ctest #8 (remhos_tests.cpp:88-92) on star-q2: the final mass to 1e-14 relative with the exact element inverse.  The run loses
    2.6 % of its mass through the moving boundary: the first known answer with a non-zero remap boundary flux (u_nbr := 0).
  * three lines of autotest 'Transport bump per-unstruct-2D' on periodic-hexagon (500 steps, 192 elements): the 10 printed digits
    of mass and max.  The max values depend on the bounds at the vertices of valence 3 and 6.  -ho 2 (CG to 1e-12) and -ho 3 are
    the exact inverse to the printed digits.
"""
import numpy as np
import pytest

from tests.unstructured_cases import KAT, oracle_run


def test_star_ctest8():
    K = KAT["star_ctest8"]["mass"]
    r, rep = oracle_run("star-q2", 1, 14, -1.0, 0.5, 5, 5, "exact")
    assert rep["steps"] == 5 and r.lat.ne == 80
    assert 5 in r.lat.valence.values()
    assert abs(r.dt - 0.06162169781886305) < 1e-15
    assert abs(r.mass0 - 0.8286020837631387) < 1e-14
    assert abs(rep["mass"] - K) <= 1e-14 * K, rep["mass"]
    assert r.mass0 - rep["mass"] > 0.02  # the mass leaves through the boundary
    # the -pa stopping rule stays within a few 1e-12 of it (the bound tests/test_gpu_unstructured.py derives for the library)
    _, rep_pa = oracle_run("star-q2", 1, 14, -1.0, 0.5, 5, 5, "pa")
    assert abs(rep_pa["mass"] - K) <= 1e-11 * K


@pytest.mark.parametrize("k", range(3))
def test_hexagon_autotest(k):
    line = KAT["hexagon"][k]
    r, rep = oracle_run("periodic-hexagon", line["rs"], line["problem"], line["dt"], line["t_final"], line["lo"], -1, "exact")
    assert rep["steps"] == 500 and r.lat.ne == 192
    assert {3, 6} <= set(r.lat.valence.values())
    assert float(f"{rep['mass']:.10g}") == line["mass"]
    assert float(f"{rep['max']:.10g}") == line["max"]


def test_face_pairing_is_symmetric():
    """every interior face is its neighbour's neighbour, with the same flip on both sides"""
    for name, rs in (("star-q2", 1), ("periodic-hexagon", 1)):
        r, _ = oracle_run(name, rs, 14 if name == "star-q2" else 0, 0.005, 0.5, 5, 1, "exact")
        m = r.lat
        e, f = np.nonzero(m.nbr >= 0)
        g, h = m.nbr[e, f], m.nface[e, f]
        assert (m.nbr[g, h] == e).all() and (m.nface[g, h] == f).all() and (m.flip[g, h] == m.flip[e, f]).all()
