#!/usr/bin/env python3
"""Records tests/golden/resident_windows_parent.npz: the resident form's final poses and traced b of the two cases of
tests/resident_windows_cases.py, from the build of the commit that later builds must reproduce bit for bit.

    git checkout <commit> -- invcompcamtrack_amd/csrc include && python __graft_entry__.py   # the build to record
    timeout -k 10 300 python tools/record_resident_windows.py [out.npz]

Both cases also go through their judges here, so a recording is never taken from a run the tests would refuse."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import resident_windows_cases as C
    import test_gpu_iter_sums as T
    from oracle import oracle as O
    O.build()
    dst = sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN
    sc, inp = C.batch_input()
    with tempfile.TemporaryDirectory() as td:
        got, out, died = C.start_batch_child(inp, td, 240)
    if died or got is None:
        raise SystemExit(f"the batch child {died or 'failed'}\n{out[-4000:]}")
    T._judge_batch(O, "515x96/slots2", sc, inp, got, "k_level_resident")
    assert "k_level_resident" in str(got["path_lv2"]), got["path_lv2"]
    _, kept = C.run_one(O)
    np.savez(dst, **C.golden_of_batch(got), **C.golden_of_one(kept))
    print(f"wrote {dst}: {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
