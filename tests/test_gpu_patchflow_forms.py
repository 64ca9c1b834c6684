"""k_patchflow in each of its four launch forms against the f64 oracle (oracle/np_patchflow.py), over the job table of
patchflow_cases.py: raw one-iteration steps against the derived bound, full runs with status and iters exact, lv_l > 0,
pyramids padded by more than psz, and a patch's independence of what else is in its launch. The far jobs of the same
module (frames up to 576 px with a displacement known in advance) hold the tap rule at coordinates of 256 and more in every
form: the one-step bound, the full-run check, the truth, continuity inside a triple of points one ulp apart, and the flow
grid on such a pair.

Group 0 (default dispatch: <1,1>, <4,1>, <8,2>) runs in this process. <16,1> needs ICTR_PF_WPP=1 and <8,2> on small patches
ICTR_PF_WPP=2; the launcher reads the variable once per process, so groups 1 and 2 each run in a fresh child process
(patchflow_child.py) that writes its results and the form of every launch to an .npz. Every check asserts the form the
launch really took (patchflow.last_form()). Run with -s to see the worst ratios (DESIGN.md records them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import patchflow_cases as PC
import patchflow_child as child

pytestmark = pytest.mark.gpu

GROUPS = (0, 1, 2)
CHILD_TIMEOUT = 240
_results = {}
_child_died = []      # groups whose child ended on a signal or its time limit


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("patchflow_children")


def _run_child(group, workdir):
    out = str(workdir / f"group{group}.npz")
    env = dict(os.environ, ICTR_PF_WPP=str(group))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(child.__file__), str(group), out], env=env,
                           timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    except subprocess.TimeoutExpired:
        _child_died.append(group)
        return f"child of group {group} ran into its time limit of {CHILD_TIMEOUT} s"
    if r.returncode < 0:
        _child_died.append(group)
    if r.returncode != 0:
        return f"child of group {group} ended with {r.returncode}:\n{r.stdout[-3000:]}"
    z = np.load(out)
    return {j.key: (z[j.key + "/new"], z[j.key + "/ok"], z[j.key + "/it"], int(z[j.key + "/form"]))
            for j in child.all_jobs(group)}


@pytest.fixture
def results(workdir):
    """get(group) -> {job key: (new, status, iters, form)}; every group runs once per session."""
    def get(group):
        if group not in _results:
            if group == 0:
                _results[0] = child.run_jobs(child.all_jobs(0))
            elif _child_died:  # (group 0 ran before any child: the groups are parametrised in order)
                pytest.skip(f"the child of group {_child_died[0]} faulted or hung: no further child is started")
            else:
                _results[group] = _run_child(group, workdir)
        if isinstance(_results[group], str):
            pytest.fail(_results[group])
        return _results[group]
    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _collect(jobs, fn):
    """Run fn(job) over the jobs, report every failure, return the worst ratio per form."""
    worst, failed = {}, []
    for job in jobs:
        try:
            r = fn(job)
        except AssertionError as e:
            failed.append(str(e)[:600])
            continue
        worst[PC.form(job)] = max(worst.get(PC.form(job), 0.0), r)
    assert not failed, "\n".join(failed)
    return worst


# ---------------------------------------------------------------- refusals
# (first in the file: it runs before any child process is started)
def test_refusals_and_the_empty_launch():
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    from invcompcamtrack_amd._lib import IctrError
    a, b = PC.pair("100x77")
    small, _ = PC.pair("67x53")
    pa, pb = ic.Pyramid(a, PC.LV, 15), ic.Pyramid(b, PC.LV, 15)
    pts = PC.interior("100x77")
    bad = {
        "psz 0": lambda: pf.track_points(pa, pb, pts, psz=0, lv_f=2),
        "psz 33": lambda: pf.track_points(ic.Pyramid(a, PC.LV, 33), ic.Pyramid(b, PC.LV, 33), pts, psz=33, lv_f=2),
        "lv_l > lv_f": lambda: pf.track_points(pa, pb, pts, psz=15, lv_f=1, lv_l=2),
        "lv_f beyond the pyramid": lambda: pf.track_points(pa, pb, pts, psz=15, lv_f=3),
        "first pyramid without gradients": lambda: pf.track_points(ic.Pyramid(a, PC.LV, 15, False), pb, pts, psz=15, lv_f=2),
        "pad < psz": lambda: pf.track_points(pa, pb, pts, psz=16, lv_f=2),
        "pyramids of different size": lambda: pf.track_points(pa, ic.Pyramid(small, PC.LV, 15), pts, psz=15, lv_f=2),
        "maxiter < 0": lambda: pf.track_points(pa, pb, pts, psz=15, lv_f=2, maxiter=-1),
    }
    for name, call in bad.items():
        with pytest.raises(IctrError):
            call()
            pytest.fail(f"{name} was accepted")
    new, ok, it = pf.track_points(pa, pb, np.zeros((0, 2), np.float32), psz=15, lv_f=2)
    assert new.shape == (0, 2) and ok.shape == (0,) and it.shape == (0,)
    assert new.dtype == np.float32 and ok.dtype == bool and it.dtype == np.int32


# ---------------------------------------------------------------- the job table
@pytest.mark.parametrize("group", GROUPS)
def test_every_launch_took_its_form(results, group):
    res = results(group)
    for key, job in PC.jobs(group).items():
        assert res[key][3] == PC.form(job), (key, res[key][3], PC.form(job))
    for key, job in PC.far_jobs(group).items():
        assert res[key][3] == PC.form(job), (key, res[key][3], PC.form(job))
    assert set(PC.GROUP_FORM[group].values()) == {res[k][3] for k in res}


def test_all_four_forms_ran(results):
    forms = {r[3] for g in GROUPS for r in results(g).values()}
    assert forms == {11, 41, 161, 82}


@pytest.mark.parametrize("group", GROUPS)
def test_one_step_within_the_derived_bound(O, results, group):
    """lv_f = lv_l = l, maxiter = 1: (new - pts) / 2^l against H^-1 b in f64, per component and point, within one_step's
    bound for the form's lane load (plus the half ulp of the f32 position that comes back)."""
    res = results(group)

    def one(job):
        new, ok, it, form = res[job.key]
        assert form == PC.form(job), job.key
        return PC.compare_step(job, new, ok, it, O)

    worst = _collect([j for j in PC.jobs(group).values() if j.kind == "step"], one)
    print(f"\ngroup {group}: device one-step error / bound, worst per form: {worst}")
    assert worst


@pytest.mark.parametrize("group", GROUPS)
def test_full_runs_equal_decisions_and_close_positions(O, results, group):
    """maxiter = 8, eps = 0.005, every level range (lv_l = 1 and 2 included), K = 1..9, the leaving points: status and
    iters equal the oracle's, positions within the tolerance of patchflow_cases.full_tolerance, lost points NaN."""
    res = results(group)

    def one(job):
        new, ok, it, form = res[job.key]
        assert form == PC.form(job), job.key
        return PC.compare_full(job, new, ok, it, O)

    worst = _collect([j for j in PC.jobs(group).values() if j.kind in ("full", "pad")], one)
    print(f"\ngroup {group}: device full-run error / (bound sum + u |new|), worst per form: {worst} "
          f"(tolerance at {PC.FULL_MARGIN * PC.FULL_FACTOR})")
    assert worst


@pytest.mark.parametrize("group", GROUPS)
def test_status_cases(O, results, group):
    """Textureless frames and psz 1 are lost at every point with no iteration; maxiter = 0 returns its input."""
    res = results(group)
    seen = 0
    for key, job in PC.jobs(group).items():
        new, ok, it, form = res[key]
        assert form == PC.form(job), key
        if job.kind == "lost" or (job.psz == 1 and job.kind in ("full", "step")):
            assert not ok.any() and np.all(it == 0) and np.isnan(new).all(), key
        elif job.kind == "maxiter0":
            _, ok_o, _, _ = PC.oracle_full(O, job)
            assert np.array_equal(ok, ok_o) and np.all(it == 0), key
            assert np.array_equal(_bits(new[ok]), _bits(job.pts[ok])) and np.isnan(new[~ok]).all(), key
        else:
            continue
        seen += 1
    assert seen >= 5


@pytest.mark.parametrize("group", GROUPS)
def test_padding_beyond_psz_gives_the_same_bits(results, group):
    res = results(group)
    for psz in PC.GROUP_FORM_PSZ[group]:
        ref = res[f"g{group}-pad0-p{psz}"]
        assert ref[1].all()
        for extra in PC.PAD_EXTRA[1:]:
            got = res[f"g{group}-pad{extra}-p{psz}"]
            assert got[3] == ref[3] == PC.GROUP_FORM[group][psz]
            assert np.array_equal(_bits(got[0]), _bits(ref[0])), (psz, extra, np.abs(got[0] - ref[0]).max())
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), (psz, extra)


@pytest.mark.parametrize("group", GROUPS)
def test_a_patch_does_not_depend_on_its_launch(results, group):
    """The full set, a permutation, every point alone and the set interleaved with lost points (in the two-wave form
    every live patch then shares its workgroup's barriers with a lost one): the same bits per point."""
    res = results(group)
    n = PC.N_INTERIOR
    for psz in PC.GROUP_FORM_PSZ[group]:
        new, ok, it, form = res[f"g{group}-pad0-p{psz}"]
        assert form == PC.GROUP_FORM[group][psz] and ok.all()
        perm = PC.perm_of(psz)
        pn, pk, pi, pf_ = res[f"g{group}-indep-perm-p{psz}"]
        assert pf_ == form and np.array_equal(_bits(pn), _bits(new[perm])) and np.array_equal(pi, it[perm]) and pk.all()
        nn, nk, ni, nf = res[f"g{group}-indep-nan-p{psz}"]
        assert nf == form and np.array_equal(_bits(nn[0::2]), _bits(new)) and np.array_equal(ni[0::2], it), psz
        assert nk[0::2].all() and not nk[1::2].any() and np.isnan(nn[1::2]).all() and np.all(ni[1::2] == 0), psz
        for k in range(n):
            on, ok1, oi, of = res[f"g{group}-indep-one{k}-p{psz}"]
            assert of == form and ok1.all()
            assert np.array_equal(_bits(on[0]), _bits(new[k])) and oi[0] == it[k], (psz, k, on[0], new[k])


# ---------------------------------------------------------------- the far jobs: coordinates of 256 and more
@pytest.mark.parametrize("group", GROUPS)
def test_far_one_step_within_the_derived_bound(O, results, group):
    """The far frames' 'step' jobs: integer centres of 40, 255, 256, 300 (512 at level 1), the values one ulp to either
    side, half-pixel and two-decimal points, each level. At an integer centre the patch is the plane's own pixels (the
    oracle's are, test_patchflow_cpu.py), so a tap pair off by one leaves the bound by orders of magnitude."""
    res = results(group)

    def one(job):
        new, ok, it, form = res[job.key]
        assert form == PC.form(job) and ok.all(), job.key
        return PC.compare_step(job, new, ok, it, O)

    worst = _collect([j for j in PC.far_jobs(group).values() if j.kind == "step"], one)
    print(f"\ngroup {group}: far frames, device one-step error / bound, worst per form: {worst}")
    assert set(worst) == {PC.GROUP_FORM[group][p] for p in PC.GROUP_FORM_PSZ[group]}


@pytest.mark.parametrize("group", GROUPS)
def test_far_full_runs_truth_and_continuity(O, results, group):
    """The far frames' full runs: status and iters equal the oracle's and positions are within compare_full's tolerance
    (one spacing of f32 at the position taken off first, see there); every point is kept and within TRUTH_BAR of the
    shift the frame was made with; the three points of a triple, one ulp apart, get displacements within 4 x the
    tolerance of each other with equal iters."""
    res = results(group)
    truth, cont = {}, [0.0]

    def one(job):
        new, ok, it, form = res[job.key]
        assert form == PC.form(job), job.key
        r = PC.compare_full(job, new, ok, it, O)
        truth[job.psz] = max(truth.get(job.psz, 0.0), PC.check_truth(job, new, ok))
        cont[0] = max(cont[0], PC.check_continuity(job, new, ok, it, O))
        return r

    worst = _collect([j for j in PC.far_jobs(group).values() if j.kind == "full"], one)
    print(f"\ngroup {group}: far frames, device full-run error beyond one spacing / (bound sum + u |new|), worst per form: "
          f"{worst}; worst truth error per psz {truth} (bars {PC.TRUTH_BAR}); largest difference inside a triple "
          f"{cont[0]:.2e} px")
    assert set(worst) == {PC.GROUP_FORM[group][p] for p in PC.GROUP_FORM_PSZ[group]}


def test_far_jobs_reached_all_four_forms(results):
    forms = {results(g)[k][3] for g in GROUPS for k in PC.far_jobs(g)}
    assert forms == {11, 41, 161, 82}


@pytest.mark.parametrize("frame", ("farx-320x64", "fary-64x320"))
def test_flow_grid_on_a_far_pair(frame):
    """FlowGrid.compute on a far pair, its dense field read at the node pixels (so after the fill): no interior node is
    lost, every interior node is within the bar of the known shift, and the nodes from 256 on are no worse than the
    others (median, factor 2). With the first tap one back at integers >= 256 every node from 256 on is a pixel off."""
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    a, b = PC.pair(frame)
    w, h = PC.frame_size(frame)
    pa, pb = ic.Pyramid(a, PC.GRID_LV, PC.GRID_PSZ), ic.Pyramid(b, PC.GRID_LV, PC.GRID_PSZ)
    g = pf.FlowGrid(w, h, PC.GRID_STEP).compute(pa, pb, psz=PC.GRID_PSZ, lv_f=PC.GRID_LV)
    assert pf.last_form() == 41
    got = PC.check_grid(frame, g.dense(), g.nodes()[1], PC.TRUTH_BAR[PC.GRID_PSZ])
    print(f"\n{frame}: device grid, largest interior error {got[0]:.4f} px, median below 256 {got[1]:.4f}, from 256 on "
          f"{got[2]:.4f}")
