"""The Remhos-side binding (include/remhos_amd/mfem_binding.hpp, the one file INTEGRATION.md asks a maintainer to add)
must at least type-check: it is compiled (-fsyntax-only) against stub declarations of exactly the MFEM and Remhos names
it uses (tests/mfem_stub/) -- MFEM itself is not in this image.  Also: the in-repo mirror of the interfaces keeps the
reference's constructor signatures and members, and agrees with the stub restatement declaration by declaration.  The same checks
against a Remhos checkout's own headers (not part of this repository): tools/check_reference_headers.py."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_header_compiles_against_stub():
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "tests", "mfem_stub"), os.path.join(ROOT, "tests", "mfem_stub", "compile_binding.cpp")]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def test_mirror_keeps_reference_signatures(tmp_path):
    """include/remhos_amd/solvers.hpp: FCTSolver(space, SmoothnessIndicator*, dt, needs_LO_prod), NeedsLOProductInput,
    CalcFCTProduct, ClipScaleSolver(space, si, dt), MassBasedAvg(space, hos, mesh_vel) -- remhos_fct.hpp:50-55, 72-86,
    139-141; remhos_lo.hpp:98-100"""
    src = tmp_path / "sig.cpp"
    src.write_text('''
#include "remhos_amd/solvers.hpp"
using namespace remhos;
void f(ParFiniteElementSpace &pfes, HOSolver &hos, const GridFunction *mv, Vector &a, Array<bool> &fl)
{
   ClipScaleSolver cs(pfes, (SmoothnessIndicator *)nullptr, 0.1);
   FCTSolver &f = cs;
   bool need = f.NeedsLOProductInput();
   (void)need;
   f.CalcFCTProduct(a, a, a, a, a, a, a, fl, fl, a);
   MassBasedAvg mba(pfes, hos, mv);
   mba.SetHOSolution(a);
   DofInfo d(pfes);
   d.ComputeElementsMinMax(a, a, a, &fl, &fl);
}
''')
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def _class_body(text, name):
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bclass\s+%s\b[^;{]*\{" % name, text)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[m.end():i - 1]


def _signatures(text, name):
    """{function name: normalised signature} of the member functions and constructors a class DECLARES at its top level:
    return type, parameter TYPES (names dropped) and cv-qualifier -- what an override has to repeat."""
    body = _class_body(text, name)
    flat, depth = [], 0
    for ch in body:  # bodies of inline functions removed
        if ch == "{":
            depth += 1
            flat.append(";")
        elif ch == "}":
            depth -= 1
        elif depth == 0:
            flat.append(ch)
    out = {}
    for stmt in "".join(flat).split(";"):
        stmt = re.sub(r"\b(public|protected|private)\s*:", " ", stmt)
        stmt = " ".join(stmt.split())
        m = re.match(r"(.*?)(~?\b\w+)\s*\(", stmt)
        if not m or m.group(2) in ("MFEM_ABORT", "MFEM_VERIFY", "RMH_VERIFY"):
            continue
        ret, fn = m.group(1).strip(), m.group(2)
        depth, j = 1, m.end()
        while depth and j < len(stmt):  # the parameter list: up to the parenthesis that closes the first one
            depth += {"(": 1, ")": -1}.get(stmt[j], 0)
            j += 1
        params, tail = stmt[m.end():j - 1], stmt[j:]
        types = []
        for prm in (params.split(",") if params.strip() else []):
            prm = re.sub(r"=.*$", "", prm).strip()                                               # default value
            prm = re.sub(r"\s*\b\w+$", "", prm) if re.search(r"[\s&*]\w+$", prm) else prm   # parameter name
            types.append(prm.replace(" ", "").replace("double", "real_t"))
        out[fn] = (ret.replace("virtual", "").replace(" ", "").replace("double", "real_t"), tuple(types),
                   bool(re.match(r"\s*const\b", tail)))
    return out


def test_mirror_signatures_equal_the_stub_restatement():
    """include/remhos_amd/solvers.hpp against the stub restatement of the reference's interfaces (tests/mfem_stub/remhos_interfaces.hpp,
    what the binding is compiled against above), declaration by declaration: every constructor and member function the stub declares
    for the abstract HOSolver / LOSolver / FCTSolver (remhos_ho.hpp:29-42, remhos_lo.hpp:28-44, remhos_fct.hpp:31-90) and for
    MassBasedAvg (remhos_lo.hpp:87-109) has the same return type, parameter types and constness in the mirror -- so the two in-repo
    restatements cannot drift apart unseen.  Both against the reference's own headers: tools/check_reference_headers.py."""
    mirror = open(os.path.join(ROOT, "include", "remhos_amd", "solvers.hpp")).read()
    stub = open(os.path.join(ROOT, "tests", "mfem_stub", "remhos_interfaces.hpp")).read()
    checked = 0
    for cls in ("HOSolver", "LOSolver", "MassBasedAvg", "FCTSolver"):
        want, got = _signatures(stub, cls), _signatures(mirror, cls)
        assert want, cls
        for fn, sig in want.items():
            assert fn in got, (cls, fn, sorted(got))
            assert got[fn] == sig, (cls, fn, got[fn], sig)
            checked += 1
    assert checked >= 15
    # the data members a caller sets through the base classes (remhos.cpp:1115-1116, 1550-1552)
    for cls, members in (("HOSolver", ["TimingData *timer"]), ("LOSolver", ["TimingData *timer"]),
                         ("FCTSolver", ["TimingData *timer", "bool verify_bounds"])):
        for text in (mirror, stub):
            body = " ".join(_class_body(text, cls).split())
            for mem in members:
                assert mem in body, (cls, mem)
