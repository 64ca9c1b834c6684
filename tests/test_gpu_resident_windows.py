"""The resident kernel's current-frame windows: the half-window fetch path alone, and both instantiations of the kernel
held to the float64 judge and to the bits of the commit before the half windows.

a. ictr_debug_half_window (k_debug_half_window, one wave) returns every lane's taps a, b, c, d of eight windows through
   the fetch path of k_level_resident's patch loop (ictr_devfn.h hw_*): the lane's own row pair by one 8-byte load, the
   pair of the row above from the lane eight below, the windows' top rows by one load per four windows. On a 24 x 17
   plane with plane[i] = i (odd row stride) every tap must be exactly the texel the definition names.
b. thirty-two patches per wave, c. sixteen patches per wave (tests/resident_windows_cases.py): every iteration's H and b
   against the judge of tests/iter_judge.py with exactly the bar of tests/test_gpu_iter_sums.py (its _judge_batch and
   _track are called, not restated), then final poses and traced b bit for bit against
   tests/golden/resident_windows_parent.npz. The blend reads the same texels and adds in the same order whichever way
   the texels reach the lane, so the bits must not move.

The golden file was recorded on an MI355X from the build of commit ec79759 (the parent of the half windows) with

    timeout -k 10 420 python tools/record_resident_windows.py tests/golden/resident_windows_parent.npz

It holds the poses of all problems and b of the first four (resident_windows_cases.KEPT).

The batch case runs in a fresh child (ICTR_RESIDENT_SLOTS is read once per process) under its own time limit; a child
that ends on a signal or at its time limit may have faulted or hung the device, so the session ends there. It is the
last case of this file.
"""
import numpy as np
import pytest

import resident_windows_cases as C
import test_gpu_iter_sums as T
from parity_util import same_bits

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120  # seconds; the child takes a few


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(C.GOLDEN))


def _taps_by_definition(plane, top_left):
    """(64, 4): a, b, c, d of the 8 x 8 pixels of the window whose top-left texel is (r0, c0) = divmod(top_left, sw)."""
    r0, c0 = divmod(int(top_left), plane.shape[1])
    r, c = np.divmod(np.arange(64), 8)
    return np.stack([plane[r0 + r + 1, c0 + c + 1], plane[r0 + r + 1, c0 + c], plane[r0 + r, c0 + c + 1],
                     plane[r0 + r, c0 + c]], axis=1)


def test_half_window_fetch_path_returns_the_texels_of_the_definition():
    from invcompcamtrack_amd import _lib
    L = _lib.load()
    rows, sw = 24, 17
    plane = np.arange(rows * sw, dtype=np.float32).reshape(rows, sw)
    # top-left texels (row, column): the first legal window (its top row is the plane's row 0), the last legal row, the
    # last legal column, both at once, and windows in between; every lane group of both top-row loads is used
    corners = [(0, 0), (rows - 9, 0), (0, sw - 9), (rows - 9, sw - 9), (0, 3), (7, 5), (1, 0), (rows - 10, sw - 10)]
    tl = np.array([r * sw + c for r, c in corners], np.int32)
    out = np.full((8, 64, 4), -1.0, np.float32)
    _lib.check(L.ictr_debug_half_window(_lib.fp(plane), rows, sw, tl.ctypes.data_as(_lib.IP), _lib.fp(out)))
    for g in range(8):
        want = _taps_by_definition(plane, tl[g])
        assert np.array_equal(out[g], want), (corners[g], np.argwhere(out[g] != want)[:8], out[g][:9], want[:9])


def _bit_equal(golden, got):
    for k, v in got.items():
        assert golden[k].shape == np.asarray(v).shape, (k, golden[k].shape, np.asarray(v).shape)
        if golden[k].dtype == np.float32:
            assert same_bits(golden[k], v), (k, np.argwhere(golden[k] != v)[:6])
        else:
            assert np.array_equal(golden[k], v), (k, np.argwhere(golden[k] != v)[:6])


def test_sixteen_patches_per_wave_8205_points(oracle, golden):
    res, kept = C.run_one(oracle)
    assert len(res) == (C.ONE_LV_F + 1) * C.ONE_MAXITER
    _bit_equal(golden, C.golden_of_one(kept))


def test_thirty_two_patches_per_wave_96_problems_two_slots(oracle, golden, tmp_path):
    sc, inp = C.batch_input()
    got, out, died = C.start_batch_child(inp, str(tmp_path), CHILD_TIMEOUT)
    if died:
        pytest.exit(f"the ICTR_RESIDENT_SLOTS={C.BATCH_SLOTS} child {died}\nno further GPU work is started in this session",
                    returncode=1)
    assert got is not None, out[-4000:]
    assert "k_level_resident" in str(got["path_lv2"]) and "k_level_resident" in str(got["path_lv0"])
    T._judge_batch(oracle, "515x96/slots2", sc, inp, got, "k_level_resident")
    _bit_equal(golden, C.golden_of_batch(got))
