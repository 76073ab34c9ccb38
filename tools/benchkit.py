"""The measuring harness of the tools/*_bench.py, stated once: a window of iterations between two device events, the per-side
figures of a series of windows, the A/B alternation every number under profiles/ was taken with, the launch counts that go with
it, the reader of a rocprofv3 kernel-stats CSV, and the tail that writes a tool's JSON document.  Workloads, arguments and
derived fields stay with each tool."""
from __future__ import annotations

import csv
import json
import os
import statistics


def window_ms(fn, iters):
    """milliseconds per call of fn over `iters` calls between two device events"""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def window_stats(times, iters, digits, count_key):
    """one side's figures: every window, their median, minimum and maximum rounded to `digits`, and the iterations per window"""
    return {"ms": [round(t, digits) for t in times], "median_ms": round(statistics.median(times), digits), "min_ms": round(min(times), digits),
            "max_ms": round(max(times), digits), count_key: iters}


def alternate(steps, warmup, min_window_s, repeats, *, calibrate, digits, count_key="iterations_per_window", window=window_ms):
    """steps: {side: fn}.  Every side in turn is warmed up (`warmup` calls) and calibrated (one window of `calibrate` calls, from
    which the iterations of a window of at least `min_window_s` follow, never fewer than `calibrate`); then `repeats` rounds over
    the sides in dict order, one window each.  -> ({side: window_stats}, {side: [ms per window]}).  `window` is a parameter so
    that the scheduling can be tested without a device."""
    iters = {}
    for name, fn in steps.items():
        for _ in range(warmup):
            fn()
        per = window(fn, calibrate)
        iters[name] = max(calibrate, int(min_window_s * 1e3 / per) + 1)
    times = {name: [] for name in steps}
    for _ in range(repeats):
        for name, fn in steps.items():
            times[name].append(window(fn, iters[name]))
    return {name: window_stats(ts, iters[name], digits, count_key) for name, ts in times.items()}, times


def with_launches(stats, steps, profiled, key="launches_per_iteration"):
    """adds to every side of `stats` its device launches per iteration over `profiled` iterations under the profiler (0: not
    measured); after the timed windows, so that the profiler is in none of them"""
    from tests.launches import launches_per_iteration
    for name, fn in steps.items():
        stats[name][key] = launches_per_iteration(fn, profiled) if profiled else "not measured"
    return stats


def library_launches(fn):
    """the library's own count of one call of fn: launches and kernel milliseconds of its forward and backward stages"""
    from tests.launches import stage_counts
    ms, cnt = stage_counts(fn)
    return {"forward": cnt[0], "backward": cnt[6], "kernel_ms_forward": round(ms[0], 4), "kernel_ms_backward": round(ms[6], 4)}


def compare(fns, a):
    """{"torch": fn, "fused": fn} of an opt-in fused path against its default: the alternation of the arguments `a` (warmup,
    min_window, repeats, profiled_iterations), both launch counts per side, and what the fused side gains"""
    doc, times = alternate(fns, a.warmup, a.min_window, a.repeats, calibrate=3, digits=4)
    with_launches(doc, fns, a.profiled_iterations)
    for name, fn in fns.items():
        doc[name]["library_launches"] = library_launches(fn)
    doc["speedup_median"] = round(doc["torch"]["median_ms"] / doc["fused"]["median_ms"], 3)
    doc["fused_faster_in_every_alternation"] = all(f < t for t, f in zip(times["torch"], times["fused"]))
    return doc


def peak_mib(fn):
    """peak device memory of one call of fn above what was allocated before it, in MiB"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def read_stats(directory):
    """(name, calls, average ns, total ns) per kernel of the last *kernel_stats.csv found under `directory`"""
    path = None
    for dirpath, _, files in os.walk(directory):
        for f in files:
            if f.endswith("kernel_stats.csv"):
                path = os.path.join(dirpath, f)
    if path is None:
        raise SystemExit(f"no kernel_stats.csv under {directory}")
    return [(row["Name"], int(row["Calls"]), float(row["AverageNs"]), float(row["TotalDurationNs"])) for row in csv.DictReader(open(path))]


def write_doc(doc, out):
    """writes the document to `out` (if given) and prints it as one line"""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(doc))
