"""Lockstep sets of coarse-to-fine flows, the part that needs no device: the C-ABI's declarations against the ctypes table
and the library's exports, the Python argument checks that come before any device call, and the CLI's --lockstep with
--host, which changes nothing. The device side is tests/test_gpu_c2fset.py."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("create", "destroy", "run", "run_rgb", "size", "last_operations", "set_timing", "get_kernel_ms")


def test_header_ctypes_table_and_exports_agree():
    """The ictr_c2fset_* functions are declared in include/ictr_c2f_set.h, which ictr.h includes inside its extern "C"
    block (ictr.h's own text declares none of them); the ctypes table is _lib.SIGNATURES_SET, with the argument counts of
    the declarations; the build lists the header and the two kernel modules; the library exports every function."""
    import __graft_entry__ as g
    with open(os.path.join(ROOT, "include", "ictr.h")) as f:
        main = f.read()
    assert main.index('#include "ictr_c2f_cost.h"') < main.index('#include "ictr_c2f_set.h"') < main.index("#ifdef __cplusplus\n}")
    assert not re.search(r"\bictr_c2fset_\w+\s*\(", main)
    with open(os.path.join(ROOT, "include", "ictr_c2f_set.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(ictr_c2fset_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(decl) == sorted("ictr_c2fset_" + n for n in NAMES)
    assert "enum { ICTR_C2FSET_MAX = 8 };" in text and pf.C2FSET_MAX == 8
    assert sorted(_lib.SIGNATURES_SET) == sorted(decl)
    for name, args in decl.items():
        assert len(_lib.SIGNATURES_SET[name][1]) == len(args.split(",")), name
    i, vp, pvp, fp = C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_float)
    assert _lib.SIGNATURES_SET["ictr_c2fset_create"] == (i, [pvp, pvp, i])
    assert _lib.SIGNATURES_SET["ictr_c2fset_run"] == _lib.SIGNATURES_SET["ictr_c2fset_run_rgb"] == (i, [vp, pvp, pvp, vp])
    assert _lib.SIGNATURES_SET["ictr_c2fset_get_kernel_ms"] == (i, [vp, fp, fp])
    assert _lib.SIGNATURES_SET["ictr_c2fset_destroy"] == (None, [vp])
    assert not set(_lib.SIGNATURES_SET) & (set(_lib.SIGNATURES) | set(_lib.SIGNATURES_COST))
    assert "ictr_c2fflow.hip" in g.SOURCES and "ictr_c2fflow_robust.hip" in g.SOURCES  # (the set's kernels are the object's)
    assert any(os.path.normpath(h).endswith(os.path.join("include", "ictr_c2f_set.h")) for h in g.HEADERS)
    lib = _lib.load()
    for name in decl:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES_SET[name][1]


def test_argument_checks_that_need_no_device():
    from invcompcamtrack_amd import stereotrack as S
    with pytest.raises(ValueError, match=r"0 members \(1 \.\. 8\)"):
        pf.CoarseToFineFlowSet([])
    with pytest.raises(ValueError, match=r"9 members \(1 \.\. 8\)"):
        pf.CoarseToFineFlowSet([None] * 9)
    with pytest.raises(TypeError, match="member 0 is a NoneType, not a CoarseToFineFlow"):
        pf.CoarseToFineFlowSet([None])
    with pytest.raises(TypeError, match="member 0 is a str"):
        pf.CoarseToFineFlowSet(["lr", "rl"])
    with pytest.raises(ValueError, match="lockstep=True needs flow='c2f' or 'c2f-1d'"):
        S.StereoPointTracker(96, 64, 4, lockstep=True)
    with pytest.raises(ValueError, match="lockstep=True needs flow='c2f' or 'c2f-1d'"):
        S.StereoPointTracker(96, 64, 4, flow="grid", lockstep=True, refine={})
    assert "CoarseToFineFlowSet" in pf.__all__
    # the C-ABI's refusals that come before the device is asked for
    L = _lib.load()
    h = C.c_void_p()
    assert L.ictr_c2fset_create(None, None, 1) != 0 and b"out is NULL" in L.ictr_last_error()
    assert L.ictr_c2fset_create(C.byref(h), None, 1) != 0 and b"members is NULL" in L.ictr_last_error()
    arr = (C.c_void_p * 9)()
    for n in (0, 9, -1):
        assert L.ictr_c2fset_create(C.byref(h), arr, n) != 0 and b"(1 .. 8)" in L.ictr_last_error()
    assert L.ictr_c2fset_create(C.byref(h), arr, 2) != 0 and b"member 0 is NULL" in L.ictr_last_error()
    assert h.value is None
    n = C.c_int(-5)
    assert L.ictr_c2fset_size(None, C.byref(n)) != 0 and L.ictr_c2fset_last_operations(None, C.byref(n)) != 0
    assert L.ictr_c2fset_set_timing(None, 1) != 0 and L.ictr_c2fset_get_kernel_ms(None, None, None) != 0
    assert L.ictr_c2fset_run(None, arr, arr, None) != 0 and b"the set is NULL" in L.ictr_last_error()
    assert L.ictr_c2fset_run_rgb(None, arr, arr, None) != 0 and n.value == -5
    L.ictr_c2fset_destroy(None)


def test_cli_lockstep_with_host_changes_nothing(tmp_path, capsys):
    from invcompcamtrack_amd import run_stereo_track as RS
    from test_stereotrack_cpu import golden
    g = golden()["two_frames"]
    fin = str(tmp_path / "in.npz")
    np.savez(fin, **{k: g[k] for k in ("disp_lr", "disp_rl", "flow_l", "flow_r")})
    out = [str(tmp_path / "host.npz"), str(tmp_path / "lockstep.npz"), str(tmp_path / "grid.npz")]
    assert RS.main(["-", out[0], "--fields", fin, "--host"]) == 0
    assert RS.main(["-", out[1], "--fields", fin, "--host", "--lockstep", "--flow", "c2f"]) == 0
    assert RS.main(["-", out[2], "--fields", fin, "--host", "--lockstep"]) == 0  # not even the flow is consulted
    with np.load(out[0]) as a:
        assert len(a["rows"]) > 0
        for o in out[1:]:
            with np.load(o) as b:
                assert b["xy_t"].tobytes() == a["xy_t"].tobytes() and b["rows"].tobytes() == a["rows"].tobytes()
    capsys.readouterr()
    with pytest.raises(SystemExit):
        RS.main(["-", out[1], "--fields", fin, "--lockstep"])  # on the device it needs the coarse-to-fine flow
    assert "--lockstep needs --flow c2f or c2f-1d" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        RS.main(["--help"])
    assert "with --host it changes nothing" in " ".join(capsys.readouterr().out.split())
