#!/usr/bin/env python3
"""Generates tests/golden/driver_refusals.json: what the driver's entry points (include/rmh_driver.h) answer to the option sets
they refuse -- the full rmhd_last_error() string of every refusal that the emulation library reaches without RCCL and without a
failing HIP call, recorded from this project's own library (tests/emu/librmh_emu.so).  tests/test_driver_refusals.py holds both
libraries to the table, whole string by whole string.

    python tests/golden/make_driver_refusals.py     # rewrites the .json file

A record is {entry, config, message}: entry is rmhd_run or rmhd_run_partitioned (null id file, device 0), config the keyword
arguments of remhos_amd.case.make_config (`mesh_file` relative to the repository), message the whole error string.  A record
with "null": "cfg" | "res" passes a null pointer for that argument instead.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "driver_refusals.json")
RUN, PART = "rmhd_run", "rmhd_run_partitioned"
STAR = "tests/golden/meshes/star-q2.mesh"

# the smallest shapes that reach the check: -rs 0, orders 2 and 4, one step
CUBE = dict(mesh="cube01_hex", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, fused=0)
PCUBE = dict(mesh="periodic-cube", rs=0, order=2, problem=10, dt=0.02, t_final=0.7, max_steps=1, fused=0)
SEG = dict(mesh="periodic-segment", rs=0, order=2, problem=0, dt=0.01, t_final=0.5, max_steps=1, fused=0)
FILE = dict(mesh="star-q2", mesh_file=STAR, rs=0, order=2, problem=14, dt=0.01, t_final=0.5, max_steps=1, fused=0)
QUAD = dict(mesh="inline-quad", rs=0, order=2, problem=14, dt=0.01, t_final=0.5, max_steps=1, fused=0)


def one(entry, base, **kw):
    return dict(entry=entry, config={**base, **kw})


def both(base, **kw):
    return [one(RUN, base, **kw), one(PART, base, **kw)]


RECORDS = (
    # ---- null arguments ----
    [dict(entry=RUN, config=CUBE, null="cfg"), dict(entry=RUN, config=CUBE, null="res"),
     dict(entry=PART, config=CUBE, null="cfg"), dict(entry=PART, config=CUBE, null="res")]
    # ---- -mono, rule by rule ----
    + both(CUBE, mono_type=2) + both(CUBE, mono_type=3) + both(CUBE, mono_type=-1)
    + [one(RUN, CUBE, mono_type=1, part=(2, 1, 1)), one(PART, CUBE, mono_type=1), one(PART, CUBE, mono_type=1, part=(2, 1, 1)),
       one(RUN, PCUBE, mono_type=1, self_wrap=1), one(RUN, CUBE, mono_type=1, fused=1), one(RUN, CUBE, mono_type=1, ps=1),
       one(RUN, CUBE, mono_type=1, ode_solver=11), one(RUN, CUBE, mono_type=1, ode_solver=13), one(RUN, CUBE, mono_type=1, dt_control=1)]
    # ---- -ho / -lo / -fct, rule by rule ----
    + both(CUBE, ho_type=5) + both(CUBE, ho_type=-1)
    + [one(RUN, CUBE, ho_type=1, part=(1, 2, 1)), one(PART, CUBE, ho_type=1, fused=1),
       one(RUN, PCUBE, ho_type=1, self_wrap=2), one(RUN, CUBE, ho_type=1, fused=1), one(RUN, CUBE, ho_type=1, pa=1),
       one(RUN, CUBE, ho_type=1, ps=1)]
    + both(CUBE, fct_type=3) + both(CUBE, fct_type=-2)
    + [one(RUN, CUBE, part=(1, 1, 2), **w) for w in (dict(fct_type=1), dict(lo_type=1), dict(lo_type=2))]
    + [one(PART, CUBE, fused=1, **w) for w in (dict(fct_type=1), dict(lo_type=1), dict(lo_type=2))]
    + [one(RUN, CUBE, fused=1, **w) for w in (dict(fct_type=1), dict(lo_type=1), dict(lo_type=2))]
    + [one(RUN, CUBE, ps=1, **w) for w in (dict(fct_type=1), dict(lo_type=1), dict(lo_type=2))]
    + [one(RUN, CUBE, fct_type=1, pa=1), one(RUN, PCUBE, fct_type=1, self_wrap=3),
       one(PART, CUBE, fct_type=4, fused=1), one(PART, CUBE, fct_type=4), one(RUN, CUBE, fct_type=4, fused=1),
       one(RUN, CUBE, fct_type=4, ps=1)]
    # ---- dim = 1, rule by rule ----
    + [one(RUN, SEG, **w) for w in (dict(ps=1), dict(ode_solver=11), dict(ode_solver=12), dict(ho_type=1), dict(lo_type=1),
                                    dict(lo_type=2), dict(fct_type=1), dict(fct_type=4), dict(mono_type=1), dict(mono_type=2),
                                    dict(part=(2, 1, 1)), dict(part=(1, 2, 1)), dict(part=(1, 1, 2)), dict(rank=1),
                                    dict(self_wrap=1), dict(save=1))]
    + [one(PART, SEG), one(PART, SEG, fused=1)]
    # ---- an unstructured mesh file, rule by rule ----
    + [one(RUN, FILE, **w) for w in (dict(part=(2, 1, 1)), dict(part=(1, 2, 1)), dict(part=(1, 1, 2)), dict(rank=1),
                                     dict(mono_type=1), dict(fused=1), dict(ho_type=1), dict(lo_type=1), dict(lo_type=2),
                                     dict(fct_type=1), dict(fct_type=4), dict(ps=1), dict(ode_solver=11), dict(ode_solver=13),
                                     dict(self_wrap=1), dict(save=1))]
    + [one(PART, FILE), one(PART, FILE, fused=1)]
    # ---- the entry points' own rules ----
    + [one(RUN, CUBE, part=(2, 1, 1)), one(RUN, CUBE, part=(2, 1, 1), fused=1), one(RUN, PCUBE, part=(1, 2, 2)),
       one(PART, CUBE), one(PART, CUBE, part=(2, 1, 1)),
       one(PART, QUAD, fused=1), one(PART, dict(QUAD, mesh="periodic-square", problem=5), fused=1)]
    # ---- the case builder's answer, handed on ----
    + both(dict(CUBE, fused=1), mesh="no-such-mesh") + both(dict(CUBE, fused=1), order=7)
    + [one(RUN, CUBE, rank=1), one(PART, QUAD, fused=1, part=(2, 1, 1)), one(PART, CUBE, fused=1, part=(64, 1, 1))]
    # ---- after build_case: orders in 3-D, product remap ----
    + [one(RUN, CUBE, lo_type=2, order=4), one(RUN, CUBE, lo_type=2, order=5), one(RUN, CUBE, mono_type=1, order=4),
       one(RUN, PCUBE, ps=1, problem=0), one(RUN, CUBE, ps=1, dt_control=1), one(RUN, CUBE, ps=1, lo_type=3),
       one(RUN, CUBE, ps=1, lo_type=4), one(RUN, dict(QUAD, problem=4), ps=1)]
    # ---- after the context exists ----
    + [one(RUN, PCUBE, self_wrap=1, fused=1), one(RUN, PCUBE, self_wrap=3, fused=1, ode_solver=0),
       one(RUN, CUBE, bounds_type=5), one(RUN, CUBE, dt_control=1), one(PART, CUBE, fused=1, bounds_type=5),
       one(PART, CUBE, fused=1, dt_control=1), one(PART, dict(CUBE, order=1), fused=1, lo_type=3)]
    # ---- two rules broken at once: which one is reported ----
    + [one(RUN, SEG, ps=1, mono_type=1), one(RUN, SEG, mono_type=2, part=(2, 1, 1)), one(RUN, SEG, pa=1, ps=1),
       one(RUN, SEG, pa=1, ho_type=5),  # (passes the dim = 1 rules: "Disabling PA / FA for 1D." is printed, then -ho is refused)
       one(RUN, SEG, rank=1, self_wrap=1), one(PART, SEG, ps=1), one(RUN, SEG, save=1, fct_type=3),
       one(RUN, FILE, fused=1, part=(2, 1, 1)), one(RUN, FILE, rank=1, mono_type=1), one(RUN, FILE, mono_type=2, fused=1),
       one(PART, FILE, mono_type=1, fused=1), one(RUN, FILE, ps=1, ode_solver=11), one(RUN, FILE, save=1, ho_type=5),
       one(RUN, CUBE, mono_type=1, fct_type=3, fused=1), one(PART, CUBE, mono_type=1, fct_type=3, fused=1),
       one(RUN, CUBE, mono_type=2, ho_type=7), one(RUN, CUBE, ho_type=1, pa=1, ps=1), one(RUN, CUBE, ho_type=1, fct_type=3, fused=1),
       # the two spellings of "partitioned": px * py * pz > 1 (-mono, -ho 1, -lo 1|2, -fct 1) does not see rank != 0, which the
       # case builder then refuses; (px > 1 || py > 1 || pz > 1 || rank != 0) (dim = 1, mesh files) does
       one(RUN, CUBE, mono_type=1, rank=1), one(RUN, CUBE, ho_type=1, rank=1), one(RUN, CUBE, fct_type=1, rank=1),
       one(RUN, CUBE, lo_type=1, rank=1, fused=1), one(RUN, SEG, rank=1, fct_type=3), one(RUN, FILE, rank=1, fct_type=3),
       one(RUN, CUBE, fct_type=1, lo_type=2, fused=1), one(RUN, CUBE, fct_type=1, pa=1, ps=1),
       one(RUN, CUBE, lo_type=2, order=4, ps=1), one(RUN, CUBE, lo_type=2, order=4, mono_type=1),
       one(RUN, CUBE, fct_type=4, fused=1, ps=1), one(PART, CUBE, fct_type=4, fused=0, ps=1),
       one(RUN, dict(CUBE, mesh="no-such-mesh"), part=(2, 1, 1)), one(PART, QUAD, fused=0), one(PART, QUAD, fct_type=3),
       one(RUN, PCUBE, ps=1, problem=0, dt_control=1, lo_type=3), one(RUN, CUBE, ps=1, dt_control=1, lo_type=3),
       one(RUN, PCUBE, self_wrap=1, fused=1, bounds_type=5)]
)


def call(lib, rec, root=ROOT):
    """run one record: (return code, message, the bytes of `res` before, the bytes after)"""
    from remhos_amd.case import RmhdResult, make_config

    kw = dict(rec["config"])
    if "part" in kw:
        kw["part"] = tuple(kw["part"])
    if kw.get("mesh_file"):
        kw["mesh_file"] = os.path.join(root, kw["mesh_file"])
    cfg, res = make_config(**kw), RmhdResult()
    C.memset(C.byref(res), 0xA5, C.sizeof(res))
    before = bytes(res)
    pc = None if rec.get("null") == "cfg" else C.byref(cfg)
    pr = None if rec.get("null") == "res" else C.byref(res)
    rc = lib.rmhd_run(pc, pr) if rec["entry"] == RUN else lib.rmhd_run_partitioned(pc, None, 0, pr)
    return rc, lib.rmhd_last_error().decode(), before, bytes(res)


def main():
    from remhos_amd.capi import load_library
    from remhos_amd.case import bind_driver
    from tests.helpers import emu_library_path

    os.environ["RMH_EXCHANGE"] = "local"
    lib = bind_driver(load_library(emu_library_path()))
    out = []
    for rec in RECORDS:
        rc, msg, _, _ = call(lib, rec)
        assert rc != 0 and msg, ("not refused", rec)
        out.append(dict(rec, message=msg))
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in out) + "\n]\n")
    print(f"{len(out)} records, {len({r['message'] for r in out})} distinct messages -> {OUT}")


if __name__ == "__main__":
    main()
