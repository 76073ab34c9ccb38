"""The C ABI of the network's Adam step (include/splatraster.h: sr_net_adam_plan / sr_net_adam_step / SrNetAdamSlot /
SR_NET_ADAM_MAX_GRADS) and what NetworkAdam refuses: exported and bound, the chunking of sr_net_adam_plan against a restatement
and a brute-force map, every bad call refused on the host with a message before any launch, the no-op cases launch nothing."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_SLOTS = 512                                                      # slots of four floats in a chunk, as in k_adam
PLAN_COUNTS = (1, 3, 4, 5, 2047, 2048, 2049, 4099, 0, 1)


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def host_floats(n=64):
    """(keep-alive, a 16-byte aligned host address): never dereferenced, every check precedes the launch"""
    buf = (C.c_float * (n + 4))()
    base = C.addressof(buf)
    return buf, base + (-base) % 16


def make_table(lib, rows):
    """rows: [(param, exp_avg, exp_avg_sq, count)] -> a planned table"""
    from splatfields_amd import _lib
    table = (_lib.SrNetAdamSlot * max(len(rows), 1))()
    for slot, (p, m, v, count) in zip(table, rows):
        slot.param, slot.exp_avg, slot.exp_avg_sq, slot.count = p, m, v, count
    assert lib.sr_net_adam_plan(table, len(rows)) == 0, lib.sr_last_error()
    return table


def scalars():
    from splatfields_amd import _lib
    return _lib.SrNetAdamScalars(1e-3, 0.03, 0.1, 0.001, 1e-15)


def call(lib, table, n_table, first, n, grads, table_dev="same", sc="default"):
    array = (C.c_void_p * max(len(grads), 1))(*grads)
    return lib.sr_net_adam_step(table, table if table_dev == "same" else table_dev, n_table, first, n, array,
                                C.byref(scalars()) if sc == "default" else sc, None)


def test_symbols_structs_and_constants_match_the_header(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    for name in ("sr_net_adam_plan", "sr_net_adam_step"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    max_grads = int(re.search(r"#define\s+SR_NET_ADAM_MAX_GRADS\s+(\d+)", header).group(1))
    assert max_grads == _lib.NET_ADAM_MAX_GRADS and max_grads >= 448
    assert C.sizeof(_lib.SrNetAdamSlot) == 3 * 8 + 2 * 8 == 40           # three pointers, two long long: no padding
    assert C.sizeof(_lib.SrNetAdamScalars) == 5 * 4

    class KernelArgument(C.Structure):     # what a step passes by value: table, range, first chunk, chunk count, scalars, gradients
        _fields_ = [("table", C.c_void_p), ("first", C.c_int), ("n", C.c_int), ("chunk0", C.c_longlong), ("chunks", C.c_longlong),
                    ("scalars", _lib.SrNetAdamScalars), ("grad", C.c_void_p * max_grads)]
    assert C.sizeof(KernelArgument) < 4096
    assert "network_adam.hip" in build.SOURCES and "adam.hip" in build.SOURCES and "adam_math.h" in build.HEADERS
    assert lib.sr_version() == 4     # additions only: no existing struct or contract changed
    for name in ("adam.hip", "network_adam.hip"):                      # one arithmetic, included by both
        assert '#include "adam_math.h"' in abi_text.source(name)
        assert "adam_element(float&" not in abi_text.source(name)
    assert "adam_element(float&" in abi_text.source("adam_math.h")
    import splatfields_amd
    for name in ("NetworkAdam", "set_network_optimizer", "network_optimizer"):
        assert hasattr(splatfields_amd, name), name


def restated_chunks(address, count):
    """slots of four floats from the 16-byte boundary at or below the parameter, 512 of them a chunk"""
    if count == 0:
        return 0
    lead = (address % 16) // 4
    slots = -(-(lead + count) // 4)
    return -(-slots // CHUNK_SLOTS)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_plan_against_a_restatement_and_a_brute_force_map(lib, offset):
    keep, base = host_floats()
    address = base + 4 * offset
    table = make_table(lib, [(address, address, address, c) for c in PLAN_COUNTS])
    ends = [table[i].chunk_end for i in range(len(PLAN_COUNTS))]
    total, want = 0, []
    for c in PLAN_COUNTS:
        total += restated_chunks(address, c)
        want.append(total)
    assert ends == want
    # brute force: every element of every tensor is in exactly one (chunk, slot), in order; chunk -> (tensor, first slot)
    owner = {}
    chunk = 0
    for i, c in enumerate(PLAN_COUNTS):
        first_chunk = chunk
        for e in range(c):
            slot = (offset + e) // 4
            owner.setdefault(first_chunk + slot // CHUNK_SLOTS, (i, slot // CHUNK_SLOTS * CHUNK_SLOTS))
            chunk = max(chunk, first_chunk + slot // CHUNK_SLOTS + 1)
    assert sorted(owner) == list(range(ends[-1]))                      # no chunk without elements, none missing
    for ch, (i, slot0) in owner.items():
        found = next(j for j, end in enumerate(ends) if end > ch)      # what the kernel's search finds
        assert found == i and (ch - (ends[i - 1] if i else 0)) * CHUNK_SLOTS == slot0, (ch, i, found)
    # the plan depends on the parameter's address and the count alone
    other = make_table(lib, [(address, base, base + 8, c) for c in PLAN_COUNTS])
    assert [other[i].chunk_end for i in range(len(PLAN_COUNTS))] == ends


def test_plan_refuses_bad_tables(lib):
    from splatfields_amd import _lib
    keep, p = host_floats()
    err = lambda: lib.sr_last_error()
    table = (_lib.SrNetAdamSlot * 2)()
    assert lib.sr_net_adam_plan(table, -1) != 0 and b"negative table length" in err()
    assert lib.sr_net_adam_plan(None, 2) != 0 and b"null pointer" in err()
    assert lib.sr_net_adam_plan(None, 0) == 0
    table[0].param, table[0].count, table[1].param = p, 4, p
    table[1].count = -1
    assert lib.sr_net_adam_plan(table, 2) != 0 and b"negative element count" in err() and b"entry 1" in err()
    table[1].count = 1 << 31
    assert lib.sr_net_adam_plan(table, 2) != 0 and b"too many elements" in err()
    table[1].count, table[1].param = (1 << 31) - 1, p + 2
    assert lib.sr_net_adam_plan(table, 2) != 0 and b"4-byte aligned" in err()
    table[1].param = p + 4
    assert lib.sr_net_adam_plan(table, 2) == 0 and table[1].chunk_end == 1 + restated_chunks(p + 4, (1 << 31) - 1)


def test_bad_steps_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    keep, p = host_floats()
    err = lambda: lib.sr_last_error()
    rows = [(p, p, p, 16), (p + 4, p + 4, p + 4, 5), (p, p, p, 3000)]
    table = make_table(lib, rows)
    g = [p, p + 4, p]
    # range
    assert call(lib, table, 3, -1, 1, g) != 0 and b"must lie inside the table" in err()
    assert call(lib, table, 3, 0, -1, g) != 0 and b"must lie inside the table" in err()
    assert call(lib, table, 3, 2, 2, g) != 0 and b"must lie inside the table" in err()
    assert call(lib, table, -1, 0, 0, g) != 0 and b"must lie inside the table" in err()
    big = make_table(lib, [(p, p, p, 1)] * (_lib.NET_ADAM_MAX_GRADS + 1))
    assert call(lib, big, len(big), 0, len(big), [p] * len(big)) != 0 and b"n must be 0 .. SR_NET_ADAM_MAX_GRADS" in err()
    # nulls
    assert lib.sr_net_adam_step(None, table, 3, 0, 3, (C.c_void_p * 3)(*g), C.byref(scalars()), None) != 0 and b"null pointer" in err() \
        and b"table_host" in err()
    assert call(lib, table, 3, 0, 3, g, table_dev=None) != 0 and b"null pointer" in err() and b"table_dev" in err()
    assert lib.sr_net_adam_step(table, table, 3, 0, 3, None, C.byref(scalars()), None) != 0 and b"grads_host" in err()
    assert call(lib, table, 3, 0, 3, g, sc=None) != 0 and b"null pointer" in err() and b"scalars" in err()
    for k, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
        broken = [list(r) for r in rows]
        broken[1][k] = None
        if name == "param":                                            # a table planned with this parameter at the boundary
            broken[1] = [None, p, p, 5]
        t = make_table(lib, [tuple(r) for r in broken])
        assert call(lib, t, 3, 0, 3, g) != 0 and b"null pointer" in err() and b"entry 1" in err(), name
        # alignment
        broken = [list(r) for r in rows]
        broken[2][k] = p + 2
        t = (_lib.SrNetAdamSlot * 3)()
        for slot, (a, m, v, c) in zip(t, broken):
            slot.param, slot.exp_avg, slot.exp_avg_sq, slot.count = a, m, v, c
        for i in range(3):
            t[i].chunk_end = table[i].chunk_end
        assert call(lib, t, 3, 0, 3, g) != 0 and b"4-byte aligned" in err() and b"entry 2" in err(), name
    assert call(lib, table, 3, 0, 3, [p, p + 6, p]) != 0 and b"4-byte aligned" in err() and b"entry 1" in err()
    assert call(lib, table, 3, 1, 2, [p + 4, p + 1]) != 0 and b"4-byte aligned" in err() and b"entry 2" in err()
    # counts
    for bad, word in ((-1, b"negative element count"), (1 << 31, b"too many elements")):
        t = make_table(lib, rows)
        t[1].count = bad
        assert call(lib, t, 3, 0, 3, g) != 0 and word in err() and b"entry 1" in err()
    # chunk_end must be what the plan fills: shifted, and computed for another alignment of the parameter
    for i in range(3):
        t = make_table(lib, rows)
        t[i].chunk_end += 1
        assert call(lib, t, 3, 0, 3, g) != 0 and b"chunk_end is not what sr_net_adam_plan fills" in err(), i
    t = make_table(lib, rows)
    t[0].chunk_end = -1
    assert call(lib, t, 3, 1, 2, g[1:]) != 0 and b"chunk_end is not what sr_net_adam_plan fills" in err() and b"entry 0" in err()
    t = make_table(lib, [(p, p, p, 2048)])
    t[0].param = p + 4                                                 # 2048 elements one float past the boundary: 2 chunks, not 1
    assert call(lib, t, 1, 0, 1, [p]) != 0 and b"chunk_end is not what sr_net_adam_plan fills" in err()


def test_nothing_to_do_launches_nothing(lib):
    """n == 0, a range whose gradients are all null and a range whose counts are all 0 are valid and return before any HIP call:
    they succeed on a host without a device, where a launch would fail."""
    keep, p = host_floats()
    assert lib.sr_net_adam_step(None, None, 0, 0, 0, None, None, None) == 0
    table = make_table(lib, [(p, p, p, 16), (p, p, p, 0), (None, None, None, 0), (p, p, p, 700)])
    assert call(lib, table, 4, 2, 0, []) == 0
    assert call(lib, table, 4, 0, 4, [None, None, None, None]) == 0
    assert call(lib, table, 4, 1, 2, [p, p]) == 0                       # counts all 0
    assert call(lib, table, 4, 0, 4, [None, p, p, None]) == 0           # a gradient only where there is nothing to step


def test_the_step_never_waits_and_uses_no_lds_and_no_atomics():
    from splatfields_amd.build import strip_comments
    text = strip_comments(abi_text.source("network_adam.hip"))        # the kernel and both entry points
    assert "k_net_adam" in text and "sr_net_adam_step" in text and "sr_net_adam_plan" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic", "__shared__",
                 "__syncthreads"):
        assert word not in text, word
    py = open(os.path.join(ROOT, "splatfields_amd", "network_optim.py")).read()
    for word in (".cpu()", "synchronize", ".tolist()", ".item()"):
        assert word not in py, word


def test_network_adam_refuses_what_splat_adam_refuses():
    from splatfields_amd import NetworkAdam
    w = torch.nn.Parameter(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="no CPU path"):
        NetworkAdam([w], lr=1e-3)
    with pytest.raises(ValueError, match="no CPU path"):
        NetworkAdam([{"params": [w], "lr": 1e-3, "name": "deform"}], lr=0.0, eps=1e-15)
    for kw in (dict(weight_decay=0.01), dict(amsgrad=True), dict(maximize=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            NetworkAdam([w], lr=1e-3, **kw)
    with pytest.raises(ValueError, match="weight_decay"):
        NetworkAdam([{"params": [w], "weight_decay": 0.1}], lr=1e-3)
    with pytest.raises(TypeError, match="unknown option"):
        NetworkAdam([w], lr=1e-3, nesterov=True)
    import inspect
    assert "visible" not in inspect.signature(NetworkAdam.step).parameters            # there is no row mask
    with pytest.raises(ValueError, match="invalid lr"):
        NetworkAdam([w], lr=-1.0)
    with pytest.raises(ValueError, match="lr must be a number"):
        NetworkAdam([w], lr=torch.tensor(1e-3))
    for bad, word in ((torch.zeros(4, 3, dtype=torch.float64), "float32"), (torch.zeros(3, 4).t(), "contiguous")):
        with pytest.raises(ValueError, match=word):
            NetworkAdam([torch.nn.Parameter(bad)], lr=1e-3)


def small_model():
    from splatfields_amd.deform_field import SplatFieldsModel
    hyper = types.SimpleNamespace(encoder_type="none", composition_rank=1, deform_d=2, rgb_d=2, flow_d=2, scale_d=2, opacity_d=2,
                                  rotation_d=2, deform_skips=[0], rgb_skips=[0], flow_skips=[0], n_frames=3)
    train = types.SimpleNamespace(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, deform_lr_max_steps=40000)
    return SplatFieldsModel(hyper, radius=None, device="cpu"), train


def test_train_setting_takes_the_optimizer_and_defaults_to_torch(monkeypatch):
    import splatfields_amd
    from splatfields_amd import network_optim
    model, train = small_model()
    assert splatfields_amd.network_optimizer() == (os.environ.get("SPLATFIELDS_NETWORK_OPTIMIZER") or "torch")
    monkeypatch.setattr(network_optim, "_NETWORK_OPTIMIZER", "torch")
    model.train_setting(train)
    assert type(model.optimizer) is torch.optim.Adam
    model.train_setting(train, optimizer="torch")
    assert type(model.optimizer) is torch.optim.Adam
    group = model.optimizer.param_groups[0]
    assert group["name"] == "deform" and group["eps"] == 1e-15 and group["lr"] == 0.00016 * 5
    with pytest.raises(ValueError, match="unknown network optimizer"):
        model.train_setting(train, optimizer="bogus")
    with pytest.raises(ValueError, match="unknown network optimizer"):
        splatfields_amd.set_network_optimizer("bogus")
    # "fused" reaches NetworkAdam, which has no CPU path: on this CPU model the choice shows in what is refused
    with pytest.raises(ValueError, match="no CPU path"):
        model.train_setting(train, optimizer="fused")
    assert splatfields_amd.set_network_optimizer("fused") == "torch" and splatfields_amd.network_optimizer() == "fused"
    with pytest.raises(ValueError, match="no CPU path"):
        model.train_setting(train)
    model.train_setting(train, optimizer="torch")                      # the argument overrides the process default
    assert type(model.optimizer) is torch.optim.Adam
    assert splatfields_amd.set_network_optimizer("torch") == "fused"


def test_the_environment_variable_sets_the_process_default():
    """read once at import: a fresh interpreter with SPLATFIELDS_NETWORK_OPTIMIZER=fused (no device is touched)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import splatfields_amd; print(splatfields_amd.network_optimizer())"
    for value, want in (("fused", "fused"), ("", "torch")):
        env = dict(os.environ, SPLATFIELDS_NETWORK_OPTIMIZER=value, PYTHONPATH=root)
        out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=root)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == want, (value, out.stdout, out.stderr)
