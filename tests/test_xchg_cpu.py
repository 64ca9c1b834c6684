"""The in-launch exchange protocol as stated in csrc/ictr_xchg.h, checked on the host (no GPU)."""
import os
import subprocess


def test_exchange_header_on_the_host(tmp_path):
    """csrc/ictr_xchg.h compiled as plain C++ (tests/cxx/xchg_hd_host.cpp, address and undefined-behaviour sanitizers).
    The program asserts: pack -> value keeps every bit of +-0, denormals, +-inf, NaNs with payload and FLT_MAX, and the
    tag test is true exactly for the packed tag; the (epoch, exchange number) pairs of the epochs 1, 2, 2^19 and 2^20 - 1
    with every exchange number 1 .. kXchgMaxSeq give distinct non-zero tags; the epoch step goes 0 -> 1 and n -> n + 1
    without clearing and 2^20 - 1 -> 1 with it; every index the team (team 2, 3, 63, 64; B 1, 3), resident (parts 1, 2,
    253, 254; slots 1, 4) and rank (world 1, 2, 16; cap 32, 64) layout functions form lies below the size function's
    granule count, no granule is addressed twice -- so the two parities never overlap -- and the size is used up. The
    sanitizers stay silent."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cxx", "xchg_hd_host.cpp")
    exe = str(tmp_path / "xchg_hd_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                        "-Werror", "-I" + os.path.join(root, "invcompcamtrack_amd", "csrc"), "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr and not r.stdout, r.stdout + r.stderr
