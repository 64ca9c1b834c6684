"""What a field source is: patchflow._device_source and its two callers, FlowRefiner._source (the descriptor that
FlowRefiner.run hands to the library) and stereotrack._descriptor, on one table of sources. No library is loaded: the
FlowGrid and the stage objects are stand-ins with a handle set by hand.

PARENT holds, per source, what the commit before the shared resolver answered: for the window (kind, on_device, x_only,
something is kept alive) and for the refiner (kind, on_device, x_only; its `keep` never outlived the call), or the name
of the exception. It was recorded by running that commit's _descriptor and FlowRefiner.run (the library call replaced by
a function that captures the descriptor) on these rows. NOW lists the cells that differ since, each with its reason:
  - a CPU tensor handed to FlowRefiner.run is refused; its host address used to be passed on as a device pointer. This is
    the one change of what is accepted or refused for a real tensor;
  - the rule for an object with data_ptr() is one rule: the dtype string ends in float32, is_cuda counts where the
    attribute exists. The window therefore accepts the duck-typed stand-in that the refiner always accepted;
  - a wrong dtype or layout is a TypeError from both callers (the refiner said ValueError); a wrong shape stays a
    ValueError."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from invcompcamtrack_amd import _lib
from invcompcamtrack_amd import patchflow as pf
from invcompcamtrack_amd import stereotrack as S

W, H = 7, 5
PLANE, FLOW, GRID = S.FIELD_PLANE, S.FIELD_FLOW, S.FIELD_GRID


class _Grid(pf.FlowGrid):
    def __init__(self, w, h):
        self._h, self.w, self.h = C.c_void_p(0x1000), w, h

    def __del__(self):
        pass


def _stage(cls, w, h):
    class Stage(cls):
        def __init__(self):
            self._h, self.w, self.h = C.c_void_p(0x2000), w, h

        def __del__(self):
            pass

        def device_ptr(self):
            return 0x3000
    return Stage()


class _Tensor:
    def __init__(self, shape, dtype="torch.float32", contiguous=True, is_cuda=None):
        self.shape, self.dtype, self._contiguous = shape, dtype, contiguous
        if is_cuda is not None:
            self.is_cuda = is_cuda

    def data_ptr(self):
        return 0x4000

    def is_contiguous(self):
        return self._contiguous


SOURCES = {
    "host plane f32": lambda: np.zeros((H, W), np.float32),
    "host flow f32": lambda: np.zeros((H, W, 2), np.float32),
    "host flow f64 exact": lambda: np.full((H, W, 2), 0.5),
    "host flow f64 inexact": lambda: np.full((H, W, 2), 0.1),
    "host wrong shape": lambda: np.zeros((H, W + 1, 2), np.float32),
    "grid": lambda: _Grid(W, H),
    "tensor flow on GPU": lambda: _Tensor((H, W, 2), is_cuda=True),
    "tensor plane on GPU": lambda: _Tensor((H, W), is_cuda=True),
    "tensor flow on CPU": lambda: _Tensor((H, W, 2), is_cuda=False),
    "stand-in flow without is_cuda": lambda: _Tensor((H, W, 2), dtype="float32"),
    "tensor wrong dtype": lambda: _Tensor((H, W, 2), dtype="torch.float64", is_cuda=True),
    "tensor not contiguous": lambda: _Tensor((H, W, 2), contiguous=False, is_cuda=True),
    "tensor wrong shape": lambda: _Tensor((H, W + 1, 2), is_cuda=True),
    "densifier wrong size": lambda: _stage(pf.FlowDensifier, W + 1, H),
    "densifier": lambda: _stage(pf.FlowDensifier, W, H),
    "refiner wrong size": lambda: _stage(pf.FlowRefiner, W + 1, H),
    "refiner": lambda: _stage(pf.FlowRefiner, W, H),
}
# source: (window, refiner) at the parent commit
PARENT = {
    "host plane f32": ((PLANE, 0, 1, True), "ValueError"),
    "host flow f32": ((FLOW, 0, 1, True), (FLOW, 0, 0)),
    "host flow f64 exact": ((FLOW, 0, 1, True), (FLOW, 0, 0)),
    "host flow f64 inexact": ("ValueError", (FLOW, 0, 0)),  # the window never rounds; the refiner takes _lib.f32c
    "host wrong shape": ("ValueError", "ValueError"),
    "grid": ((GRID, 0, 1, True), (GRID, 0, 0)),
    "tensor flow on GPU": ((FLOW, 1, 1, True), (FLOW, 1, 0)),
    "tensor plane on GPU": ((PLANE, 1, 1, True), "ValueError"),
    "tensor flow on CPU": ("TypeError", (FLOW, 1, 0)),
    "stand-in flow without is_cuda": ("TypeError", (FLOW, 1, 0)),
    "tensor wrong dtype": ("TypeError", "ValueError"),
    "tensor not contiguous": ("TypeError", "ValueError"),
    "tensor wrong shape": ("ValueError", "ValueError"),
    "densifier wrong size": ("ValueError", "ValueError"),
    "densifier": ((FLOW, 1, 1, True), (FLOW, 1, 0)),
    "refiner wrong size": ("ValueError", "TypeError"),  # no stage source of the refiner: it goes to np.asarray
    "refiner": ((FLOW, 1, 1, True), "TypeError"),
}
# (source, caller): the cells that differ from PARENT on purpose (the module docstring)
NOW = {
    ("tensor flow on CPU", "refiner"): "TypeError",  # the deliberate tightening
    ("stand-in flow without is_cuda", "window"): (FLOW, 1, 1, True),
    ("tensor wrong dtype", "refiner"): "TypeError",
    ("tensor not contiguous", "refiner"): "TypeError",
}


def _outcome(fn):
    try:
        return fn()
    except (TypeError, ValueError) as e:
        return type(e).__name__


def _window(src):
    d, keep = S._descriptor(src, True, W, H)
    return d.kind, d.on_device, d.x_only, keep is not None


def _refiner(src):
    f, _ = _stage(pf.FlowRefiner, W, H)._source(src)
    assert f.sign == 1
    return f.kind, f.on_device, f.x_only


def test_the_table_is_complete():
    assert set(PARENT) == set(SOURCES) and {k for k, _ in NOW} <= set(SOURCES)


@pytest.mark.parametrize("name", SOURCES)
def test_both_callers_answer_as_the_parent_did(name):
    for k, (caller, fn) in enumerate((("window", _window), ("refiner", _refiner))):
        got = _outcome(lambda: fn(SOURCES[name]()))
        want = NOW.get((name, caller), PARENT[name][k])
        print(name, caller, got, "(parent:", PARENT[name][k], ")")
        assert got == want, (name, caller)


@pytest.mark.parametrize("name", SOURCES)
def test_the_resolver(name):
    """None for a host array; else the kind, the pointer, the source itself to keep alive, and the components."""
    src = SOURCES[name]()
    got = _outcome(lambda: pf._device_source(src, W, H, (pf.FlowRefiner, pf.FlowDensifier)))
    if isinstance(src, np.ndarray):
        assert got is None
    elif isinstance(got, str):
        assert got == NOW.get((name, "window"), PARENT[name][0])
    else:
        kind, ptr, keep, components = got
        assert keep is src and components == (1 if kind == PLANE else 2)
        assert ptr == {_Grid: 0x1000, _Tensor: 0x4000}.get(type(src), 0x3000)
        assert (kind, int(kind != GRID)) == NOW.get((name, "window"), PARENT[name][0])[:2]
    # a stage class that the caller does not accept is no device source
    if name.startswith("refiner"):
        assert pf._device_source(src, W, H, (pf.FlowDensifier,)) is None


def test_a_sign_of_2_and_the_windows_own_host_rule():
    with pytest.raises(ValueError):
        S.field(np.zeros((H, W), np.float32), 2)
    d, keep = S._descriptor(S.field(np.full((H, W), 0.5), -1), False, W, H)
    assert (d.sign, d.x_only, d.kind, keep.dtype) == (-1, 0, PLANE, np.float32)
    assert _lib.FIELD_GRID == GRID
