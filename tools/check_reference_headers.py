"""The binding against a Remhos checkout's OWN headers -- what tests/ cannot do, because those headers are not part of this repository
(tests/test_binding_compiles.py checks the same against the stub restatement under tests/mfem_stub/):

  1. include/remhos_amd/mfem_binding.hpp behind the checkout's remhos_ho.hpp / remhos_lo.hpp / remhos_fct.hpp / remhos_tools.hpp
     (only mfem.hpp and general/forall.hpp stubbed) must type-check (tests/mfem_stub/compile_binding_ref.cpp);
  2. every virtual function and constructor of the abstract HOSolver / LOSolver / FCTSolver (remhos_ho.hpp:29-42, remhos_lo.hpp:28-44,
     remhos_fct.hpp:31-90) and of the concrete MassBasedAvg / ClipScaleSolver (remhos_lo.hpp:87-109, remhos_fct.hpp:137-155) has the
     same return type, parameter types and constness in the mirror (include/remhos_amd/solvers.hpp) and in the stub restatement.

    python tools/check_reference_headers.py <remhos checkout>      (exit 1 on a failure)
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.test_binding_compiles import _signatures  # noqa: E402

# non-virtual helpers of the reference's implementation, folded into kernels here (rmh_lo_massavg, rmh_fct_product)
HELPERS = ("MassesAndVolumesAtPosition", "CalcCompatibleLOProduct", "ScaleProductBounds")


def main():
    if len(sys.argv) != 2 or not os.path.exists(os.path.join(sys.argv[1], "remhos_fct.hpp")):
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", ref,
           "-I", os.path.join(ROOT, "tests", "mfem_stub"), os.path.join(ROOT, "tests", "mfem_stub", "compile_binding_ref.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    print("binding behind the checkout's headers:", "compiles" if p.returncode == 0 else "FAILS\n" + p.stderr[-3000:])
    bad = [] if p.returncode == 0 else ["compile"]
    mirror = open(os.path.join(ROOT, "include", "remhos_amd", "solvers.hpp")).read()
    stub = open(os.path.join(ROOT, "tests", "mfem_stub", "remhos_interfaces.hpp")).read()
    checked = 0
    for header, classes in (("remhos_ho.hpp", ["HOSolver"]), ("remhos_lo.hpp", ["LOSolver", "MassBasedAvg"]),
                            ("remhos_fct.hpp", ["FCTSolver", "ClipScaleSolver"])):
        text = open(os.path.join(ref, header)).read()
        for cls in classes:
            for other, label in ((mirror, "solvers.hpp"), (stub, "remhos_interfaces.hpp")):
                if label == "remhos_interfaces.hpp" and cls == "ClipScaleSolver":
                    continue  # (the stub restates the abstract classes and MassBasedAvg only)
                got = _signatures(other, cls)
                for fn, sig in _signatures(text, cls).items():
                    if fn.startswith("~") or fn in HELPERS:
                        continue
                    checked += 1
                    if got.get(fn) != sig:
                        bad.append(f"{label} {cls}::{fn}: {got.get(fn)} != {sig}")
    print(f"declarations compared: {checked}")
    for b in bad:
        print("DIFFERS:", b)
    return 1 if bad or checked < 20 else 0


if __name__ == "__main__":
    sys.exit(main())
