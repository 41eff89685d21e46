"""fct_projection_kernel (remhos_amd/csrc/rmh_efp.hpp) under host sanitizers, the way tests/test_sanitizers.py runs the other
kernels: the emulation built with -fsanitize=address,undefined (out-of-range LDS / global indexing) and with -fsanitize=thread
(every LDS hand-off between work-items that no barrier orders -- the row buffers, the ratios handed from pass 1 to pass 2),
p = 2 in 3-D and p = 3 in 2-D.

    python -m pytest tests -m sanitizer            (opt-in: minutes)
"""
import pytest

from tests import test_sanitizers as base

pytestmark = pytest.mark.sanitizer

SELECTED = ["tests/test_efp_emu.py::test_projection_kernel_vs_oracle[cube01_hex-0-2-10-0.3]",
            "tests/test_efp_emu.py::test_projection_kernel_vs_oracle[inline-quad-1-3-14-0.3]"]


@pytest.fixture(autouse=True)
def _select(monkeypatch):
    monkeypatch.setattr(base, "SELECTED", SELECTED)


def test_projection_under_asan_ubsan():
    base.test_emulation_under_asan_ubsan()


def test_projection_under_tsan():
    base.test_emulation_under_tsan()
