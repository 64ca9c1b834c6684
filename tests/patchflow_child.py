"""Runs the patch-flow jobs of one group of patchflow_cases (its table and its far jobs) on the device and keeps what came
back.

Imported by test_gpu_patchflow_forms.py for group 0 (default dispatch). Groups 1 and 2 need ICTR_PF_WPP=1 / 2, which
launch_patchflow reads once per process, so the test starts this file as a fresh process for each:

    ICTR_PF_WPP=<group> python patchflow_child.py <group> <out.npz>

The .npz holds, per job key, new / status / iters / form (patchflow.last_form() right after the job's launch).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import patchflow_cases as PC  # noqa: E402


def run_jobs(jobs):
    """{key: (new (K,2) f32, status (K,) bool, iters (K,) i32, form)} for an iterable of PC.Job."""
    import invcompcamtrack_amd as ic
    from invcompcamtrack_amd import patchflow as pf
    pyr, out = {}, {}
    for job in jobs:
        if (job.frame, job.pad) not in pyr:
            a, b = PC.pair(job.frame)
            pyr[job.frame, job.pad] = (ic.Pyramid(a, PC.LV, job.pad), ic.Pyramid(b, PC.LV, job.pad))
        pa, pb = pyr[job.frame, job.pad]
        new, ok, it = pf.track_points(pa, pb, job.pts, psz=job.psz, lv_f=job.lv_f, lv_l=job.lv_l, maxiter=job.maxiter,
                                      eps=PC.EPS)
        out[job.key] = (new, ok, it, pf.last_form())
    return out


def all_jobs(group):
    """The group's job table, then its far jobs (patchflow_cases.far_jobs): one process runs both."""
    return list(PC.jobs(group).values()) + list(PC.far_jobs(group).values())


def main(argv):
    group, path = int(argv[1]), argv[2]
    if os.environ.get("ICTR_PF_WPP") != str(group):
        raise SystemExit(f"ICTR_PF_WPP must be {group} for group {group}")
    flat = {}
    for key, (new, ok, it, form) in run_jobs(all_jobs(group)).items():
        flat[key + "/new"], flat[key + "/ok"], flat[key + "/it"], flat[key + "/form"] = new, ok, it, np.int32(form)
    np.savez(path, **flat)


if __name__ == "__main__":
    main(sys.argv)
