"""RANSAC pose sampling pinned per trial: k_ransac_hyp and k_ransac_score<16 / 32 / 64> through
ictr_debug_ransac_trials against the host restatement (itself judged against mpmath in test_ransac_mp_cpu.py), bit for
bit, at every tile and at chunk sizes with tails; then whole runs (select rounds, the host's early stop, chunk and round
boundaries, the post-filter, a reused sampler) against sample_poses_host, bit for bit."""
import functools

import numpy as np
import pytest

import ransac_cases as K
from invcompcamtrack_amd import ransac as R

pytestmark = pytest.mark.gpu

TRIALS = 300  # per case: 18 tiles of 16 + 12, 9 of 32 + 12, 4 of 64 + 44; chunks of 16 (19), 100 (3) and one of 300


def _sampler(monkeypatch, case, smax, tile=None, chunk=None):
    """Both variables are read at creation."""
    for k, v in (("ICTR_RANSAC_TILE", tile), ("ICTR_RANSAC_CHUNK", chunk)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    s = R.RansacSampler(case["x"].shape[1], smax)
    if chunk is not None:
        assert s.chunk == chunk
    s.set_points(case["x"], case["X"])
    return s


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _trials_equal(dev, host, what):
    """status and draws of every trial, hyp, cnt and words of the status-1 trials: the same bits."""
    assert np.array_equal(dev["status"], host["status"]), what
    assert np.array_equal(dev["draws"], host["draws"]), what
    ok = host["status"] == 1
    bad = np.nonzero(np.any(_bits(dev["hyp"][ok]) != _bits(host["hyp"][ok]), axis=1))[0]
    if bad.size:
        print("\n%s: hyp differs on %d of %d status-1 trials, first %d, max |diff| %.3e"
              % (what, bad.size, int(ok.sum()), int(np.nonzero(ok)[0][bad[0]]),
                 np.nanmax(np.abs(dev["hyp"][ok][bad] - host["hyp"][ok][bad]))))
    assert bad.size == 0, what
    assert np.array_equal(dev["cnt"][ok], host["cnt"][ok]), what
    assert np.array_equal(dev["words"][ok], host["words"][ok]), what


# ---------------------------------------------------------------- a. every trial
@pytest.mark.parametrize("chunk", [None, 16, 100, 1000])
@pytest.mark.parametrize("tile", [16, 32, 64])
def test_every_trial_device_equals_host(monkeypatch, tile, chunk):
    for case in K.all_cases():
        host = K.host_trials_cached(case["name"], 0, TRIALS)
        s = _sampler(monkeypatch, case, 1, tile, chunk)
        dev = s.debug_trials(case["fc"], case["cc"], case["thr"], case["kc"], case["seed"], 0, TRIALS)
        _trials_equal(dev, host, "%s tile %d chunk %s" % (case["name"], tile, chunk))
        if case["name"].startswith("random") and case["x"].shape[1] >= 63:
            assert int(host["status"].sum()) > TRIALS // 2  # the comparison of hyp, cnt and words is not empty


@pytest.mark.parametrize("name", ["random-n4-r1-kc0", "random-n65-r1-kc-0.05", "random-n257-r0.6-kc0", "mirror"])
def test_trial_windows_across_2_31_and_2_32(monkeypatch, name):
    """Trials 2^31 - 8 .. 2^31 + 7 and 2^32 - 8 .. 2^32 + 7 against the host, and the period of the draw stream:
    (t << 32) | k is taken in 64 bits, so trial 2^32 + j is trial j."""
    case = {c["name"]: c for c in K.all_cases()}[name]
    s = _sampler(monkeypatch, case, 1, None, 16)
    cam = (case["fc"], case["cc"], case["thr"], case["kc"], case["seed"])
    for first in ((1 << 31) - 8, (1 << 32) - 8):
        dev = s.debug_trials(*cam, first, 16)
        _trials_equal(dev, K.host_trials_cached(name, first, 16), "%s from %d" % (name, first))
    low, high = s.debug_trials(*cam, 0, 8), s.debug_trials(*cam, 1 << 32, 8)
    assert np.array_equal(low["status"], high["status"]) and np.array_equal(low["draws"], high["draws"])
    ok = low["status"] == 1
    for k in ("hyp", "cnt", "words"):
        assert low[k][ok].tobytes() == high[k][ok].tobytes(), k
    mid = s.debug_trials(*cam, 1 << 31, 8)
    if case["x"].shape[1] > 4:  # (at N = 4 the draws differ only in their order)
        assert not np.array_equal(np.sort(mid["draws"], 1), np.sort(low["draws"], 1))


def test_debug_trials_refusals_and_no_trace_in_the_next_run(monkeypatch):
    import invcompcamtrack_amd as ic
    case = K.random_case(65, 1.0, -0.05)
    monkeypatch.delenv("ICTR_RANSAC_CHUNK", raising=False)
    s = R.RansacSampler(65, 8)
    cam = (case["fc"], case["cc"], case["thr"], case["kc"], case["seed"])
    with pytest.raises(ic.IctrError):  # before set_points
        s.debug_trials(*cam, 0, 4)
    s.set_points(case["x"], case["X"])
    for first, count in ((0, 0), (-1, 4), (0, (1 << 20) + 1), ((1 << 40) - 3, 4)):
        with pytest.raises(ic.IctrError):
            s.debug_trials(*cam, first, count)
    with pytest.raises(ic.IctrError):
        s.debug_trials(case["fc"], case["cc"], float("nan"), case["kc"], case["seed"], 0, 4)
    s.run_async(case["fc"], case["cc"], 8, 100000, case["thr"], case["kc"], case["seed"])
    with pytest.raises(ic.IctrError):  # refused while the run is in flight, as the setters are
        s.debug_trials(*cam, 0, 4)
    first = s.wait()
    s.debug_trials(*cam, 1000, 50)
    s.run_async(case["fc"], case["cc"], 8, 100000, case["thr"], case["kc"], case["seed"])
    _same(s.wait(), first)


# ---------------------------------------------------------------- b. whole runs
def _same(dev, host):
    """tests/test_gpu_ransac.py::_same with p, R and t held to the bits: the per-trial tests above hold R and t to the
    bits, and p is the same se3_log<double> of the same G on both sides."""
    assert dev["accepted"] == host["accepted"] and dev["trials_used"] == host["trials_used"]
    assert np.array_equal(dev["trials"], host["trials"]) and np.array_equal(dev["draws"], host["draws"])
    assert len(dev["p"]) == len(host["p"])
    for k in ("p", "R", "t"):
        assert dev[k].shape == host[k].shape and dev[k].tobytes() == host[k].tobytes(), k
    assert len(dev["inl"]) == len(host["inl"])
    assert all(np.array_equal(a, b) for a, b in zip(dev["inl"], host["inl"]))
    assert np.array_equal(dev["inl_cnt"], host["inl_cnt"])


_BY_NAME = None


def _case(name):
    global _BY_NAME
    if _BY_NAME is None:
        _BY_NAME = {c["name"]: c for c in K.all_cases()}
    return _BY_NAME[name]


@functools.lru_cache(maxsize=None)
def _host_run(name, nsamples, maxtrials, seed=None, thr=None):
    c = _case(name)
    return R.sample_poses_host(c["x"], c["X"], c["fc"], c["cc"], nsamples, maxtrials, c["thr"] if thr is None else thr,
                               c["kc"], c["seed"] if seed is None else seed, detail=True)


def _dev_run(monkeypatch, name, nsamples, maxtrials, tile, chunk, seed=None, thr=None):
    c = _case(name)
    s = _sampler(monkeypatch, c, nsamples, tile, chunk)
    s.run_async(c["fc"], c["cc"], nsamples, maxtrials, c["thr"] if thr is None else thr, c["kc"],
                c["seed"] if seed is None else seed)
    return s.wait()


SPARSE = "random-n129-r0.3-kc-0.05"  # a success every few dozen trials: runs of a thousand trials and more


@pytest.mark.parametrize("tile", [16, 64])
def test_runs_in_chunks_of_16_around_the_early_stop(monkeypatch, tile):
    """The host reads `done` after every group of 64 chunks: samples found before chunk 64, between chunks 64 and 128
    (the second group must run, the third must not matter), and maxtrials binding at no multiple of 16."""
    acc = _host_run(SPARSE, 100000, 2600)["accepted_trials"]
    before = int(np.searchsorted(acc, 1000))          # acc[before - 1] < 1000 <= 63 * 16 + 15
    between = int(np.searchsorted(acc, 1500)) + 1     # 1024 <= acc[between - 1] < 2048
    assert before >= 4 and acc[before - 1] < 1024 <= 1500 <= acc[between - 1] < 2048, (before, between, acc[:between])
    for ns, maxtrials in ((before, 2600), (between, 2600), (100000, 1501), (100000, 2045)):
        host = _host_run(SPARSE, ns, maxtrials)
        if ns == 100000:
            assert host["trials_used"] == maxtrials and 0 < host["accepted"] < ns
        _same(_dev_run(monkeypatch, SPARSE, ns, maxtrials, tile, 16), host)


@pytest.mark.parametrize("tile", [16, 64])
def test_completing_success_on_a_chunk_boundary(monkeypatch, tile):
    """trials_used = base + sLast + 1 with the nsamples-th success the last trial of a chunk, then the first trial of the
    next chunk; chunk and nsamples are chosen from the host's accepted trials."""
    acc = [int(t) for t in _host_run(SPARSE, 100000, 2600)["accepted_trials"]]
    picks = {}
    for ns in range(4, len(acc) + 1):
        t = acc[ns - 1]
        for kind, m in (("last", t + 1), ("first", t)):
            ks = [k for k in range(17, 200) if m % k == 0 and m // k >= 2 and k % 16]
            if ks and kind not in picks:
                picks[kind] = (ns, ks[0], t)
    assert set(picks) == {"last", "first"}, picks
    for kind, (ns, chunk, t) in picks.items():
        assert (t + 1) % chunk == 0 if kind == "last" else t % chunk == 0
        host = _host_run(SPARSE, ns, 2600)
        assert host["trials_used"] == t + 1 and host["accepted"] == ns
        _same(_dev_run(monkeypatch, SPARSE, ns, 2600, tile, chunk), host)


DENSE = "random-n64-r1-kc0.05"


@functools.lru_cache(maxsize=None)
def _dense_case():
    """N = 64, every match true: nearly every trial succeeds, so one chunk of 4096 holds thousands of successes."""
    x, X = K.matches(64, 1.0, 0.05, seed=1064)
    return K._case(DENSE, x, X, 0.05)


def test_select_rounds_inside_one_chunk(monkeypatch):
    """Chunk 4096, maxtrials 3000: k_ransac_select walks three rounds of 1024 trials and carries `held` forward.
    nsamples 1024, 1025 and 2500, and the two values that put the completing success on trial 1023 (the last of round
    0) and on trial 1024 (the first of round 1)."""
    c = _dense_case()
    full = R.sample_poses_host(c["x"], c["X"], c["fc"], c["cc"], 3000, 3000, c["thr"], c["kc"], c["seed"], detail=True)
    acc = [int(t) for t in full["accepted_trials"]]
    assert len(acc) > 2500 and 1023 in acc and 1024 in acc, len(acc)
    s = _sampler(monkeypatch, c, 3000, 32, 4096)
    for ns in (1024, 1025, 2500, acc.index(1023) + 1, acc.index(1024) + 1, 3000):
        # the host's run of ns samples is the prefix of the full run; its post-filter is taken anew
        keep, cnt = R._post_filter([np.nonzero(b)[0] for b in _dense_bits(full)[:min(ns, len(acc))]], 64)
        used = acc[ns - 1] + 1 if ns <= len(acc) else 3000
        s.run_async(c["fc"], c["cc"], ns, 3000, c["thr"], c["kc"], c["seed"])
        dev = s.wait()
        assert dev["accepted"] == min(ns, len(acc)) and dev["trials_used"] == used, ns
        assert np.array_equal(dev["trials"], np.asarray(acc)[keep]), ns
        assert np.array_equal(dev["inl_cnt"], cnt), ns
        sel = _dense_rows(full)[keep]
        for k in ("p", "R", "t"):
            assert dev[k].tobytes() == np.ascontiguousarray(full[k][sel]).tobytes(), (ns, k)
        assert all(np.array_equal(dev["inl"][i], full["inl"][j]) for i, j in enumerate(sel)), ns


def _dense_rows(full):
    """Row of `full` (post-filtered) for every accepted sample of the full run; the full run must have lost none."""
    assert len(full["p"]) == full["accepted"]
    return np.arange(full["accepted"])


def _dense_bits(full):
    bits = np.zeros((full["accepted"], 64), bool)
    for s, ids in enumerate(full["inl"]):
        bits[s, ids] = True
    return bits


@pytest.mark.parametrize("tile", [16, 64])
def test_post_filter_drops_exactly_the_named_samples(monkeypatch, tile):
    """Matches 0 .. 5 are outliers among N = 40 and S = 24 < N: the post-filter drops sample s when inl_cnt[s] <= 4,
    the rule restated here from the per-trial record of the host."""
    ns, n = 24, 40
    host = _host_run("postfilter", ns, 3000)
    dev = _dev_run(monkeypatch, "postfilter", ns, 3000, tile, 100)
    _same(dev, host)
    assert dev["accepted"] == ns and 0 < len(dev["p"]) < dev["accepted"]
    rec = K.host_trials_cached("postfilter", 0, dev["trials_used"])
    succ = np.nonzero((rec["status"] == 1) & (rec["cnt"] >= 4))[0][:ns]
    assert len(succ) == ns and succ[-1] + 1 == dev["trials_used"]
    bits = (rec["words"][succ, 0][:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)
    inl_cnt = bits.sum(0)
    dropped = [s for s in range(ns) if inl_cnt[s] <= 4]
    assert dropped and set(dropped) <= set(range(6)), dropped  # only the outlier matches' indices are flagged
    assert np.array_equal(dev["trials"], np.delete(succ, dropped))
    assert np.array_equal(dev["inl_cnt"], inl_cnt[inl_cnt > 4])


def test_one_sampler_run_three_times(monkeypatch):
    """Only the state header of the output block is cleared between runs: a run after a larger one, with another seed
    and threshold, and one on a non-null stream, each equal a fresh sampler's (and the host's)."""
    import torch
    c = _case(SPARSE)
    s = _sampler(monkeypatch, c, 40, None, 100)
    s.run_async(c["fc"], c["cc"], 40, 2600, c["thr"], c["kc"], c["seed"])
    _same(s.wait(), _host_run(SPARSE, 40, 2600))
    s.run_async(c["fc"], c["cc"], 7, 2600, 3.5, c["kc"], 99)
    second = s.wait()
    _same(second, _host_run(SPARSE, 7, 2600, 99, 3.5))
    fresh = _dev_run(monkeypatch, SPARSE, 7, 2600, None, 100, 99, 3.5)
    for k in ("p", "R", "t", "inl_cnt", "trials", "draws", "words"):
        assert second[k].tobytes() == fresh[k].tobytes(), k
    stream = torch.cuda.Stream()
    s.run_async(c["fc"], c["cc"], 23, 2600, 1.0, c["kc"], 3, stream=stream)
    third = s.wait()
    _same(third, _host_run(SPARSE, 23, 2600, 3, 1.0))
    fresh = _dev_run(monkeypatch, SPARSE, 23, 2600, None, 100, 3, 1.0)
    for k in ("p", "R", "t", "inl_cnt", "trials", "draws", "words"):
        assert third[k].tobytes() == fresh[k].tobytes(), k
