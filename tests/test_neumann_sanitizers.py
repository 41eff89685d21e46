"""The kernels of remhos_amd/csrc/rmh_neumann.hpp (-ho 1) under host sanitizers, the way tests/test_pdu_sanitizers.py runs the
preconditioned upwind kernel: the emulation built with -fsanitize=address,undefined (out-of-range LDS / global indexing in the
contraction buffers, the face tables and the scratch vectors of the context) and with -fsanitize=thread (every LDS hand-off
between two contractions has its barrier), at p = 3 in 3-D with and without a second pass, p = 6 in 2-D, and u = 0.

    python -m pytest tests -m sanitizer            (opt-in: minutes)
"""
import pytest

from tests import test_sanitizers as base

pytestmark = pytest.mark.sanitizer

SELECTED = ["tests/test_neumann_emu.py::test_ho_neumann_vs_oracle[cube01_hex-0-3-10-0.3]",
            "tests/test_neumann_emu.py::test_ho_neumann_vs_oracle[inline-quad-1-6-14-0.3]",
            "tests/test_neumann_emu.py::test_ho_neumann_vs_oracle[inline-quad-1-1-14-0.3-unperturbed]",
            "tests/test_neumann_emu.py::test_ho_neumann_zero_input"]


@pytest.fixture(autouse=True)
def _select(monkeypatch):
    monkeypatch.setattr(base, "SELECTED", SELECTED)


def test_neumann_under_asan_ubsan():
    base.test_emulation_under_asan_ubsan()


def test_neumann_under_tsan():
    base.test_emulation_under_tsan()
