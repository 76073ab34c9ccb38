"""The two ways this project counts launches, each stated once: the library's own per-stage count (sr_profile_collect) and the
device records of torch.profiler.  Both need a HIP device.  Which records belong to a kernel under test is the caller's filter."""
import ctypes as C

import torch


def stage_counts(fn):
    """-> (ms, counts) per profile stage of the library while fn runs, as lists.  Profiling is switched off again even if fn
    raises."""
    from splatfields_amd import _lib
    lib = _lib.load()
    ms, cnt = (C.c_double * _lib.PROFILE_STAGES)(), (C.c_longlong * _lib.PROFILE_STAGES)()
    lib.sr_profile_collect(ms, cnt)                                         # drop whatever was recorded before
    ms, cnt = (C.c_double * _lib.PROFILE_STAGES)(), (C.c_longlong * _lib.PROFILE_STAGES)()
    lib.sr_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.sr_profile_enable(0)
    lib.sr_profile_collect(ms, cnt)
    return list(ms), list(cnt)


def device_events(fn, iters=1, drop_host_ranges=False):
    """Every device record (kernel, copy, fill) of the profiler while fn runs `iters` times.  The host activity is on as well:
    with the device activity alone the trace loses records.
    drop_host_ranges: a record_function range of the host (torch wraps Optimizer.step in one) is mirrored on the device's time
    line under its own name: that is no device work, and is left out.  Kernels, copies and fills have no host record of their
    name."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    host = {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CPU} if drop_host_ranges else ()
    return [e for e in prof.events() if e.device_type != torch.autograd.DeviceType.CPU and e.name not in host]


def device_records(fn, iters=1, drop_host_ranges=False):
    """the names of device_events"""
    return [e.name for e in device_events(fn, iters, drop_host_ranges)]


def launches_per_iteration(fn, iters):
    """Device kernel records per iteration, copies and fills excluded: all of them, and the library's ("sr::" in the name).  None
    where the profiler records no device kernel."""
    names = [n for n in device_records(fn, iters) if not n.startswith(("Memcpy", "Memset"))]
    if not names:
        return None
    return {"all": round(len(names) / iters, 2), "library": round(sum(1 for n in names if "sr::" in n) / iters, 2)}
