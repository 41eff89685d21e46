"""lo_upwind_prec_kernel (remhos_amd/csrc/rmh_pdu.hpp) under host sanitizers, the way tests/test_efp_sanitizers.py runs the
projection kernel: the emulation built with -fsanitize=address,undefined (out-of-range LDS / global indexing: the dense matrix,
the packed Cholesky factor, the triangular solves), p = 2 in 3-D and p = 3 in 2-D.

    python -m pytest tests -m sanitizer            (opt-in: minutes)
"""
import pytest

from tests import test_sanitizers as base

pytestmark = pytest.mark.sanitizer

SELECTED = ["tests/test_pdu_emu.py::test_lo_upwind_prec_vs_oracle[cube01_hex-0-2-10-0.3]",
            "tests/test_pdu_emu.py::test_lo_upwind_prec_vs_oracle[inline-quad-1-3-14-0.3]"]


@pytest.fixture(autouse=True)
def _select(monkeypatch):
    monkeypatch.setattr(base, "SELECTED", SELECTED)


def test_lo_upwind_prec_under_asan_ubsan():
    base.test_emulation_under_asan_ubsan()
