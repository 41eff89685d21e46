"""Unstructured 2-D quadrilateral meshes on the device: the checks of tests/unstructured_cases.py (CPU twins on the emulation build:
tests/test_unstructured_emu.py), the reference's known answers on star-q2 and periodic-hexagon
(tests/golden/reference_kat_unstructured.json) through the driver, and the shipped binary on the reference's ctest #8 line."""
import os
import re
import subprocess

import pytest

from tests import unstructured_cases as uc
from tests.test_unstructured_emu import check_entry_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return uc.Backend(True)


@pytest.mark.parametrize("p", [1, 3, 6])
def test_rotated_elements_give_the_lattice_numbers(dev, p):
    uc.check_rotated(dev, p)


@pytest.mark.parametrize("name,valences", [("star-q2", (5,)), ("periodic-hexagon", (3, 6))])
def test_bounds_at_irregular_vertices(dev, name, valences):
    uc.check_bounds_irregular(dev, name, valences)


@pytest.mark.parametrize("name", ["star-q2", "periodic-hexagon"])
@pytest.mark.parametrize("rs", [0, 1])
def test_lumped_mass_against_restatement(dev, name, rs):
    uc.check_lumped_mass(dev, name, rs)


def test_hexagon_dt_control(dev):
    """-bt 1 -dtc 1 on a file mesh: the steps that are too large are repeated as in the restatement.  (Not with -vb: the LO update of
    such a step leaves its bounds -- what the estimate detects -- and the reference's check aborts on it.)"""
    uc.check_run(dev, "periodic-hexagon", 0, 4, 6, dt=uc.DTC_DT, bounds_type=1, dt_control=1)


def test_hexagon_verify_bounds(dev):
    """-vb on a file mesh: the in-loop bounds checks of the LO and the limited update pass at the reference's step"""
    uc.check_run(dev, "periodic-hexagon", 0, 4, 6, verify_bounds=1)


@pytest.mark.parametrize("pa", [0, 1])
def test_star_steps_against_restatement(dev, pa):
    uc.check_run(dev, "star-q2", pa, 5, 5)


@pytest.mark.parametrize("lo", [3, 4, 5])
def test_hexagon_steps_against_restatement(dev, lo):
    uc.check_run(dev, "periodic-hexagon", 0, lo, 6)


@pytest.mark.parametrize("k", range(3))
def test_hexagon_known_answers(dev, k):
    """autotest 'Transport bump per-unstruct-2D': 500 steps, the 10 printed digits of mass and max"""
    uc.check_kat_hexagon(dev, k)


@pytest.mark.parametrize("pa", [0, 1])
def test_star_ctest8(dev, pa):
    """remhos_tests.cpp:88-92.  pa = 0: 1e-12 relative; pa = 1: plus the distance of the restatement's own -pa run"""
    uc.check_kat_star(dev, pa)


def test_entry_points_refuse_an_unstructured_context(dev):
    check_entry_refusals(dev)


def test_binary_runs_the_reference_line():
    """the reference's ctest #8 command line, verbatim but for the path of the mesh file"""
    exe = os.path.join(uc.uo.ROOT, "remhos_amd", "remhos_amd_run")
    line = uc.KAT["star_ctest8"]
    args = line["args"].replace("./data/star-q2.mesh", uc.mesh_path("star-q2")).split()
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    mass = float(re.search(r"Final mass u:\s+(\S+)", out.stdout).group(1))
    assert mass == float(f"{line['mass']:.10g}"), out.stdout
    assert "time step: 5," in out.stdout
