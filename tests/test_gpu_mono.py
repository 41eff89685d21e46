"""MonoRDSolver (-mono 1) on the MI355X: mono_rd_kernel (remhos_amd/csrc/rmh_mono.hpp) against the restatement of tests/mono_oracle.py
on the inputs, shapes and tolerances of tests/test_mono_emu.py (whose check functions run here with the device library), the
driver's -mono 1 path over ten steps, its refusals, and the shipped executable."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_mono_emu import (CASES_ML, CASES_NOML, check_follows_the_moved_mesh, check_mass_lim, check_no_mass_lim, check_refusals,
                                 check_run_10_steps)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "remhos_amd", "remhos_amd_run")


@pytest.fixture(scope="module")
def lib():
    import torch

    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver

    assert torch.cuda.is_available()
    return bind_driver(load_library())


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # (a copy: the shared reference arrays are read-only)


@pytest.mark.parametrize("mesh,rs,p,prob", CASES_NOML)
def test_mono_no_mass_lim_gpu(lib, mesh, rs, p, prob):
    check_no_mass_lim(lib, mesh, rs, p, prob, to_dev=_dev)


@pytest.mark.parametrize("mesh,rs,p,prob", CASES_ML)
def test_mono_mass_lim_gpu(lib, mesh, rs, p, prob):
    check_mass_lim(lib, mesh, rs, p, prob, to_dev=_dev, second=True)


def test_mono_follows_the_moved_mesh_gpu(lib):
    check_follows_the_moved_mesh(lib, to_dev=_dev)


@pytest.mark.parametrize("rs,p", [(0, 1), (1, 2), (1, 3)])
def test_driver_mono_run_10_steps_gpu(lib, rs, p):
    check_run_10_steps(lib, rs, p)


def test_driver_mono_refusals_gpu(lib):
    check_refusals(lib)


def test_binary_mono(lib):
    """remhos_amd_run -mono 1 -vb as a child process: rc 0, the printed mass is rmhd_run's; -mono 2 and -si are refused"""
    from remhos_amd.case import RmhdResult, make_config

    args = ["-m", "data/inline-quad.mesh", "-p", "14", "-rs", "1", "-o", "2", "-dt", "0.002", "-tf", "0.7", "-ms", "3"]
    p = subprocess.run([EXE] + args + ["-mono", "1", "-vb"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    cfg = make_config("inline-quad", 1, 2, 14, 0.002, 0.7, max_steps=3, fused=0, mono_type=1)
    res = RmhdResult()
    assert lib.rmhd_run(C.byref(cfg), C.byref(res)) == 0, lib.rmhd_last_error()
    m = re.search(r"^Final mass u:\s*([-+0-9.eE]+)\s*$", p.stdout, re.M)
    assert m, p.stdout
    assert float(m.group(1)) == float(f"{res.final_mass:.10g}")
    assert int(re.search(r"time step: (\d+)", p.stdout).group(1)) == 3
    for extra, word in ((["-mono", "2"], "-mono 2"), (["-mono", "1", "-si", "1"], "-si")):
        q = subprocess.run([EXE] + args + extra, capture_output=True, text=True, timeout=60)
        assert q.returncode == 1 and word in q.stderr, (q.returncode, q.stderr)
