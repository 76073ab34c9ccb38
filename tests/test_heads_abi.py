"""The C ABI of the grouped head networks (include/splatraster.h: sr_mlp_chain_group[_bf16], sr_mlp_group_*): declared,
exported and bound with matching signatures, structs and constants, additions only, every bad call refused on the host with a
message before any launch, empty calls succeed."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_mlp_chain_group", "sr_mlp_chain_group_bf16", "sr_mlp_group_input_forward", "sr_mlp_group_input_backward", "sr_mlp_group_output",
       "sr_mlp_group_top_gradient")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_with_matching_signatures(lib):
    from splatfields_amd import _lib
    header = abi_text.header()
    for name in NEW:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define SR_VERSION 4\b", header)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SR_MLP_(?:GROUP|OUT)_[A-Z0-9_]+)\s+(\d+)\b", header, re.M)}
    assert defs == {"SR_MLP_GROUP_MAX_NETS": _lib.MLP_GROUP_MAX_NETS, "SR_MLP_GROUP_MAX_OPS": _lib.MLP_GROUP_MAX_OPS,
                    "SR_MLP_GROUP_MAX_HEADS": _lib.MLP_GROUP_MAX_HEADS, "SR_MLP_OUT_NONE": _lib.MLP_OUT_NONE,
                    "SR_MLP_OUT_SIGMOID": _lib.MLP_OUT_SIGMOID, "SR_MLP_OUT_NORMALIZE": _lib.MLP_OUT_NORMALIZE}
    assert (_lib.MLP_GROUP_MAX_NETS, _lib.MLP_GROUP_MAX_OPS, _lib.MLP_GROUP_MAX_HEADS) == (8, 40, 8)
    # the op table of a group is a kernel argument: n_nets, first[], the ops, n_points and the slope stay under 4 KB
    assert C.sizeof(_lib.SrMlpOp) == 96
    assert 4 * (2 + _lib.MLP_GROUP_MAX_NETS) + _lib.MLP_GROUP_MAX_OPS * C.sizeof(_lib.SrMlpOp) + 8 < 4096
    assert re.search(r"static_assert\(sizeof\(MlpGroupK\)[^;]*4096", abi_text.source("mlp.hip"))
    for cls, size in ((_lib.SrMlpNet, 16), (_lib.SrMlpHeadInput, 24), (_lib.SrMlpHeadOutput, 48)):      # the field order: test_c_abi.py
        assert C.sizeof(cls) == size and cls.__name__ in abi_text.structs()
    import splatfields_amd
    assert callable(splatfields_amd.set_heads) and callable(splatfields_amd.heads)


def test_additions_only():
    """the structs and limits of the existing chain entry points are what they were"""
    from splatfields_amd import _lib
    header = abi_text.header()
    assert re.search(r"#define SR_MLP_MAX_OPS 24\b", header) and re.search(r"#define SR_MLP_MAX_PACK_JOBS 32\b", header)
    assert (_lib.MLP_MAX_OPS, _lib.MLP_MAX_PACK_JOBS, _lib.RESFIELD_MAX_JOBS) == (24, 32, 16)
    assert C.sizeof(_lib.SrMlpPackJob) == 80
    for old in ("sr_mlp_chain", "sr_mlp_chain_bf16", "sr_mlp_pack", "sr_mlp_pack_bf16", "sr_mlp_input_forward", "sr_mlp_input_backward",
                "sr_mlp_top_gradient", "sr_mlp_weight_grad"):
        assert re.search(r"^int %s\(" % old, header, re.M) and old in _lib.SYMBOLS


def aligned_buffer():
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    return buf, base


def good_op(base, **kw):
    from splatfields_amd import _lib
    op = _lib.SrMlpOp()
    op.w_packed, op.bias, op.src, op.store = base, base, base, base
    op.out_tiles, op.mem_tiles, op.reg_tiles, op.src_row, op.epilogue = 4, 2, 0, 32, _lib.MLP_LEAKY
    op.store_row, op.store_channels = 64, 64
    for k, v in kw.items():
        setattr(op, k, v)
    return op


@pytest.mark.parametrize("entry", ["sr_mlp_chain_group", "sr_mlp_chain_group_bf16"])
def test_chain_group_refuses_bad_calls_and_launches_nothing(lib, entry):
    from splatfields_amd import _lib
    keep, base = aligned_buffer()
    fn = getattr(lib, entry)
    err = lambda: lib.sr_last_error()

    def call(n=10, ht=4, ops_per_net=(2, 1), n_nets=None, nets=-1, slope=0.01, **op_kw):
        tables = []
        table = (_lib.SrMlpNet * max(len(ops_per_net), 1))()
        for y, cnt in enumerate(ops_per_net):
            arr = (_lib.SrMlpOp * max(cnt, 1))()
            for j in range(cnt):
                arr[j] = good_op(base, **(op_kw if (y, j) == (len(ops_per_net) - 1, cnt - 1) else {}))
            tables.append(arr)
            table[y].ops, table[y].n_ops = C.cast(arr, C.POINTER(_lib.SrMlpOp)), cnt
        return fn(n, ht, len(ops_per_net) if n_nets is None else n_nets, table if nets == -1 else nets, slope, None)

    for kw, msg in ((dict(n=-1), b"n_points"), (dict(ht=5), b"hidden_tiles"), (dict(ht=0), b"hidden_tiles"), (dict(ht=16), b"hidden_tiles"),
                    (dict(n_nets=-1), b"SR_MLP_GROUP_MAX_NETS"), (dict(ops_per_net=(1,) * 9), b"SR_MLP_GROUP_MAX_NETS"),
                    (dict(nets=None), b"null net table"), (dict(ops_per_net=(2, 0)), b"at least one op"),
                    (dict(ops_per_net=(20, 20, 1)), b"SR_MLP_GROUP_MAX_OPS"), (dict(ops_per_net=(24, 17)), b"SR_MLP_GROUP_MAX_OPS"),
                    (dict(slope=1.0), b"negative_slope"), (dict(slope=-0.1), b"negative_slope"), (dict(slope=float("nan")), b"negative_slope"),
                    # what sr_mlp_chain refuses in an op, in the last op of the last net: counts and tile parities, rows, alignment
                    (dict(out_tiles=0), b"unsupported op"), (dict(out_tiles=5), b"unsupported op"), (dict(mem_tiles=1, reg_tiles=1), b"unsupported op"),
                    (dict(mem_tiles=0, reg_tiles=0), b"unsupported op"), (dict(reg_tiles=6), b"unsupported op"), (dict(mem_tiles=-2), b"unsupported op"),
                    (dict(w_packed=None), b"unsupported op"), (dict(w_packed=base + 4), b"unsupported op"), (dict(bias=base + 8), b"unsupported op"),
                    (dict(src=None), b"unsupported op"), (dict(src_row=16), b"unsupported op"), (dict(src_row=34), b"unsupported op"),
                    (dict(src=base + 4), b"unsupported op"), (dict(epilogue=3), b"unsupported op"), (dict(epilogue=_lib.MLP_MASK), b"unsupported op"),
                    (dict(epilogue=_lib.MLP_MASK, mask=base, mask_row=32), b"unsupported op"), (dict(mask_bits=base + 2), b"unsupported op"),
                    (dict(sign_store=base + 1), b"unsupported op"), (dict(store_channels=0), b"unsupported op"),
                    (dict(store_channels=65, store_row=80), b"unsupported op"), (dict(store_row=32), b"unsupported op")):
        assert call(**kw) != 0 and msg in err() and entry.encode() in err(), (kw, err())
    # the limits themselves are fine, and so are the alternatives an op may use: all validated, nothing to launch
    for kw in (dict(ops_per_net=(1,) * 8), dict(ops_per_net=(24, 16)), dict(ht=8, out_tiles=8, reg_tiles=8), dict(slope=0.0),
               dict(epilogue=_lib.MLP_MASK, mask_bits=base), dict(epilogue=_lib.MLP_MASK, mask=base, mask_row=64), dict(bias=None), dict(store=None)):
        assert call(n=0, **kw) == 0, (kw, err())
    assert call(ops_per_net=(), nets=None) == 0 and call(n=0, ops_per_net=(), nets=None) == 0            # no nets: valid, nothing is launched
    assert call(n=0, ht=5) != 0 and call(n=0, out_tiles=5) != 0                                           # an empty call is still validated


def head_inputs(base, rows, multires, x0=-1, dx0=-1):
    from splatfields_amd import _lib
    t = (_lib.SrMlpHeadInput * max(len(rows), 1))()
    for i, (r, L) in enumerate(zip(rows, multires)):
        t[i].row, t[i].multires = r, L
        t[i].x0 = base if x0 == -1 else x0
        t[i].dL_dx0 = base if dx0 == -1 else dx0
    return t


def test_group_input_kernels_refuse_bad_calls_and_launch_nothing(lib):
    keep, base = aligned_buffer()
    p = C.c_void_p(base)
    err = lambda: lib.sr_last_error()

    def fwd(n=10, rows=(96, 64), multires=(4, 3), nh=None, heads=-1, F=16, TL=3, xyz=p, feat=p, time=p, **kw):
        t = head_inputs(base, rows, multires, **kw) if heads == -1 else heads
        return lib.sr_mlp_group_input_forward(n, len(rows) if nh is None else nh, t, F, TL, xyz, feat, time, None)

    def bwd(n=10, rows=(96, 64), multires=(4, 3), nh=None, heads=-1, F=16, xyz=p, dxyz=p, dfeat=p, **kw):
        t = head_inputs(base, rows, multires, **kw) if heads == -1 else heads
        return lib.sr_mlp_group_input_backward(n, len(rows) if nh is None else nh, t, F, xyz, dxyz, dfeat, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(n=-1), b"n_points"), (dict(nh=-1), b"SR_MLP_GROUP_MAX_HEADS"), (dict(rows=(96,) * 9, multires=(4,) * 9), b"SR_MLP_GROUP_MAX_HEADS"),
                        (dict(heads=None), b"null head table"), (dict(F=-1), b"n_features"), (dict(multires=(17, 3)), b"multires"),
                        (dict(multires=(4, -1)), b"multires"), (dict(rows=(96, 66)), b"row must be"), (dict(rows=(96, 32)), b"row must be"),
                        (dict(rows=(0, 64)), b"row must be"), (dict(xyz=None), b"null pointer")):
            assert call(**kw) != 0 and msg in err() and b"sr_mlp_group_input_" in err(), (call.__name__, kw, err())
        assert call(n=0, xyz=None) == 0 and call(rows=(), multires=(), heads=None, xyz=None) == 0       # empty: valid, nothing is launched
        assert call(n=0, multires=(17, 3)) != 0                                                           # ... but still validated
    for kw, msg in ((dict(TL=-1), b"time_multires"), (dict(TL=17), b"time_multires"), (dict(x0=None), b"null pointer in the head table"),
                    (dict(x0=base + 4), b"16-byte aligned"), (dict(feat=None), b"null pointer"), (dict(rows=(96, 40)), b"row must be")):
        assert fwd(**kw) != 0 and msg in err(), (kw, err())
    assert fwd(n=0, rows=(96, 40), time=None) == 0                  # without a time the row need not hold its encoding
    for kw, msg in ((dict(dx0=None), b"null pointer in the head table"), (dict(dx0=base + 8), b"16-byte aligned")):
        assert bwd(**kw) != 0 and msg in err(), (kw, err())
    assert bwd(dxyz=None, dfeat=None, xyz=None) == 0                # nothing asked for: nothing is launched


def test_group_output_kernels_refuse_bad_calls_and_launch_nothing(lib):
    from splatfields_amd import _lib
    keep, base = aligned_buffer()
    err = lambda: lib.sr_last_error()

    def table(outs=(3, 1, 4), rows=(32, 32, 32), acts=(0, 1, 2), **kw):
        t = (_lib.SrMlpHeadOutput * max(len(outs), 1))()
        for i, (o, r, a) in enumerate(zip(outs, rows, acts)):
            t[i].y, t[i].out, t[i].dL_dout, t[i].g = base, base, base, base
            t[i].out_features, t[i].row, t[i].activation = o, r, a
            if i == len(outs) - 1:
                for k, v in kw.items():
                    setattr(t[i], k, v)
        return t

    def out(n=10, nh=None, heads=-1, **kw):
        t = table(**kw) if heads == -1 else heads
        return lib.sr_mlp_group_output(n, len(kw.get("outs", (3, 1, 4))) if nh is None else nh, t, None)

    def top(n=10, nh=None, heads=-1, slope=0.01, **kw):
        t = table(**kw) if heads == -1 else heads
        return lib.sr_mlp_group_top_gradient(n, len(kw.get("outs", (3, 1, 4))) if nh is None else nh, t, slope, None)

    for call in (out, top):
        for kw, msg in ((dict(n=-1), b"n_points"), (dict(nh=-1), b"SR_MLP_GROUP_MAX_HEADS"), (dict(nh=9), b"SR_MLP_GROUP_MAX_HEADS"),
                        (dict(heads=None), b"null head table"), (dict(outs=(3, 1, 0)), b"out_features"), (dict(outs=(3, 1, 129), rows=(32, 32, 160)), b"out_features"),
                        (dict(acts=(0, 1, 3)), b"unknown output activation"), (dict(acts=(0, 1, -1)), b"unknown output activation"),
                        (dict(y=None), b"null pointer in the head table"), (dict(y=base + 2), b"4-byte aligned")):
            assert call(**kw) != 0 and msg in err() and b"sr_mlp_group_" in err(), (call.__name__, kw, err())
        assert call(n=0) == 0 and call(nh=0, heads=None) == 0                                            # empty: valid, nothing is launched
        assert call(n=0, acts=(0, 1, 3)) != 0
    assert out(out=None) != 0 and b"null pointer in the head table" in err()
    assert out(n=0, g=None, dL_dout=None, rows=(0, 0, 0)) == 0         # the output kernel reads neither
    for kw, msg in ((dict(g=None), b"null pointer in the head table"), (dict(g=base + 4), b"16-byte aligned"), (dict(rows=(32, 32, 2)), b"row must be"),
                    (dict(rows=(32, 32, 30)), b"row must be"), (dict(dL_dout=base + 1), b"4-byte aligned"), (dict(slope=1.0), b"negative_slope"),
                    (dict(slope=float("nan")), b"negative_slope")):
        assert top(**kw) != 0 and msg in err(), (kw, err())
    assert top(n=0, dL_dout=None, out=None) == 0                       # a head without a gradient is valid


def test_nothing_waits_for_the_device_and_nothing_is_added_atomically():
    from splatfields_amd.build import strip_comments
    code = strip_comments(abi_text.source("mlp.hip"))
    start = code.index("struct GroupInK")
    small = code[start:]
    for kernel in ("k_mlp_group_input_forward", "k_mlp_group_input_backward", "k_mlp_group_output", "k_mlp_group_top_gradient"):
        assert small.count("hipLaunchKernelGGL(%s," % kernel) == 1, kernel       # one launch each
    assert small.count("hipLaunchKernelGGL") == 4
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic"):
        assert word not in code, word
    for word in ("rsqrt", "__fdividef", "__sinf", "__cosf", "__expf", "sinf(", "cosf(", "expf("):      # double arithmetic in the small kernels
        assert word not in small, word
    # the chain bodies exist once each: the group kernels and the single-net kernels call the same device functions
    assert code.count("void mlp_chain_body(") == 1 and code.count("mlp_chain_body<HT>(") == 2
    assert code.count("void mlp_chain_body_bf16(") == 1 and code.count("mlp_chain_body_bf16<HT>(") == 2
    assert code.count("__builtin_amdgcn_mfma_f32_16x16x32_bf16") == 2 and code.count("lds_copy_wait();") == 4
    py = open(os.path.join(ROOT, "splatfields_amd", "fused_mlp.py")).read()
    grouped = py[py.index("# ---- the head networks of a step as groups"):]
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in grouped, word
