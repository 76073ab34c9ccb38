"""The C ABI of the fused flow head (include/splatraster.h: sr_flow_head_*): declared, exported and bound with matching
signatures and constants, additions only, every bad call refused on the host with a message before any launch, and the
selection of the path (keyword > set_flow_head > SPLATFIELDS_FLOW_HEAD > "torch")."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_flow_head_saved_bytes", "sr_flow_head_workspace_bytes", "sr_flow_head_dz_row", "sr_flow_head_forward", "sr_flow_head_backward")
OFFSET, SE3, SE3_AFFINE, SE3_SCALED, AFFINE, DCT = range(6)
ROWS = {OFFSET: (3,), SE3: (3, 3), SE3_AFFINE: (3, 3, 3), SE3_SCALED: (3, 3, 1, 3), AFFINE: (9, 3)}


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_with_matching_signatures(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    assert "flow_head.hip" in build.SOURCES
    for name in NEW:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define SR_VERSION 4\b", header)
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SR_FLOW_[A-Z0-9_]+)\s+(\d+)\b", header, re.M)}
    assert defs == {"SR_FLOW_OFFSET": _lib.FLOW_OFFSET, "SR_FLOW_SE3": _lib.FLOW_SE3, "SR_FLOW_SE3_AFFINE": _lib.FLOW_SE3_AFFINE,
                    "SR_FLOW_SE3_SCALED": _lib.FLOW_SE3_SCALED, "SR_FLOW_AFFINE": _lib.FLOW_AFFINE, "SR_FLOW_DCT": _lib.FLOW_DCT,
                    "SR_FLOW_MAX_BRANCHES": _lib.FLOW_MAX_BRANCHES, "SR_FLOW_MAX_WIDTH": _lib.FLOW_MAX_WIDTH,
                    "SR_FLOW_MAX_OUT": _lib.FLOW_MAX_OUT, "SR_FLOW_MAX_BASIS": _lib.FLOW_MAX_BASIS}
    assert (_lib.FLOW_OFFSET, _lib.FLOW_SE3, _lib.FLOW_SE3_AFFINE, _lib.FLOW_SE3_SCALED, _lib.FLOW_AFFINE, _lib.FLOW_DCT) == tuple(range(6))
    assert 3 * _lib.FLOW_MAX_BASIS <= _lib.FLOW_MAX_OUT and (_lib.FLOW_MAX_WIDTH, _lib.FLOW_MAX_BASIS) == (256, 10)
    # struct SrFlowBranch: two pointers and an int, padded to 24 bytes
    assert C.sizeof(_lib.SrFlowBranch) == 24 and [f[0] for f in _lib.SrFlowBranch._fields_] == ["weight", "bias", "rows"]
    import splatfields_amd
    for name in ("set_flow_head", "flow_head_path", "fused_flow_head"):
        assert callable(getattr(splatfields_amd, name)), name


def test_size_queries(lib):
    from splatfields_amd.flow_head import MODELS, branch_rows
    for model, rows in ROWS.items():
        assert lib.sr_flow_head_dz_row(model, 0) == sum((r + 3) // 4 * 4 for r in rows), model
    for k in range(1, 11):
        assert lib.sr_flow_head_dz_row(DCT, k) == (3 * k + 3) // 4 * 4
    for name, (code, _) in MODELS.items():      # the Python restatement of the branch table
        assert sum((r + 3) // 4 * 4 for r in branch_rows(name, 4)) == lib.sr_flow_head_dz_row(code, 4), name
    assert lib.sr_flow_head_dz_row(DCT, 0) == 0 and lib.sr_flow_head_dz_row(DCT, 11) == 0 and lib.sr_flow_head_dz_row(6, 4) == 0 and \
        lib.sr_flow_head_dz_row(-1, 4) == 0
    for n in (1, 1000, 100_000):
        assert lib.sr_flow_head_saved_bytes(SE3, n, 128, 0) >= 6 * 8 * n and lib.sr_flow_head_saved_bytes(SE3, n, 128, 0) % 256 == 0
        assert lib.sr_flow_head_saved_bytes(DCT, n, 128, 10) >= 30 * 8 * n
        assert lib.sr_flow_head_workspace_bytes(DCT, n, 128, 4) >= (n + 255) // 256 * 4 * 8
        assert lib.sr_flow_head_workspace_bytes(SE3, n, 128, 0) > 0       # never 0 for a supported shape
    for query in (lib.sr_flow_head_saved_bytes, lib.sr_flow_head_workspace_bytes):
        assert query(SE3, 0, 128, 0) > 0                                  # an empty call is supported
        for bad in ((SE3, 100, 130, 0), (SE3, 100, 0, 0), (SE3, 100, 260, 0), (SE3, 100, -4, 0), (SE3, -1, 128, 0), (SE3, 1 << 31, 128, 0),
                    (6, 100, 128, 4), (-1, 100, 128, 4), (DCT, 100, 128, 0), (DCT, 100, 128, 11)):
            assert query(*bad) == 0, bad
        assert query(SE3, 100, 256, 0) > 0 and query(SE3, 100, 4, 0) > 0 and query(DCT, 100, 128, 10) > 0


def test_bad_calls_are_refused_on_the_host_and_empty_ones_launch_nothing(lib):
    from splatfields_amd import _lib
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd4, odd2 = C.c_void_p(base), C.c_void_p(base + 4), C.c_void_p(base + 2)      # host memory: never dereferenced
    err = lambda: lib.sr_last_error()

    def table(rows, weight=base, bias=base):
        t = (_lib.SrFlowBranch * max(len(rows), 1))()
        for i, r in enumerate(rows):
            t[i].weight, t[i].bias, t[i].rows = weight, bias, r
        return t

    def fwd(model=SE3, n=10, width=128, k=0, rows=None, nb=None, branches=-1, hidden=p, pts=p, bases=p, means=p, flow=p, saved=p):
        rows = ROWS.get(model, (3 * k,)) if rows is None else rows
        t = table(rows) if branches == -1 else branches
        return lib.sr_flow_head_forward(model, n, width, k, len(rows) if nb is None else nb, t, hidden, pts, bases, means, flow, saved, None)

    def bwd(model=SE3, n=10, width=128, k=0, rows=None, nb=None, branches=-1, pts=p, bases=p, saved=p, gm=p, gf=p, dp=p, dz=p, dh=p, ws=p):
        rows = ROWS.get(model, (3 * k,)) if rows is None else rows
        t = table(rows, bias=None) if branches == -1 else branches
        return lib.sr_flow_head_backward(model, n, width, k, len(rows) if nb is None else nb, t, pts, bases, saved, gm, gf, dp, dz, dh, ws, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(width=130), b"multiple of 4"), (dict(width=260), b"multiple of 4"), (dict(width=0), b"multiple of 4"),
                        (dict(model=7), b"unknown flow model"), (dict(model=-1), b"unknown flow model"), (dict(n=-1), b"n_points"),
                        (dict(n=1 << 31), b"n_points"), (dict(model=DCT, k=0), b"n_basis"), (dict(model=DCT, k=11), b"n_basis"),
                        (dict(rows=(3,)), b"wrong number of branches"), (dict(rows=(3, 3, 3)), b"wrong number of branches"),
                        (dict(nb=5), b"wrong number of branches"), (dict(rows=(3, 4)), b"wrong branch rows"),
                        (dict(model=AFFINE, rows=(3, 9)), b"wrong branch rows"), (dict(model=DCT, k=4, rows=(9,)), b"wrong branch rows"),
                        (dict(model=SE3_SCALED, rows=(3, 3, 3, 1)), b"wrong branch rows"), (dict(branches=None), b"wrong number of branches"),
                        (dict(branches=table((3, 3), weight=None)), b"null pointer"), (dict(branches=table((3, 3), weight=base + 4)), b"16-byte aligned"),
                        (dict(pts=None), b"null pointer"), (dict(model=DCT, k=4, bases=None), b"reads bases"), (dict(pts=odd2), b"aligned"),
                        (dict(saved=odd4), b"aligned")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
        assert call(n=0, pts=None, saved=None) == 0                       # no points: valid, nothing is launched
    for kw, msg in ((dict(hidden=None), b"null pointer"), (dict(means=None), b"null pointer"), (dict(flow=None), b"null pointer"),
                    (dict(hidden=odd4), b"16-byte aligned"), (dict(flow=odd4), b"16-byte aligned"), (dict(branches=table((3, 3), bias=None)), b"null pointer")):
        assert fwd(**kw) != 0 and msg in err(), (kw, err())
    for kw, msg in ((dict(saved=None), b"null pointer"), (dict(gm=None), b"null pointer"), (dict(dz=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(dz=odd4), b"16-byte aligned"), (dict(dh=odd4), b"16-byte aligned"), (dict(gf=odd2), b"aligned")):
        assert bwd(**kw) != 0 and msg in err(), (kw, err())


def test_nothing_waits_for_the_device_and_nothing_is_added_atomically():
    from splatfields_amd.build import strip_comments
    code = strip_comments(abi_text.source("flow_head.hip"))
    entries = "\n".join(abi_text.entry_point(name) for name in NEW)
    assert "k_flow_head_forward" in code and "k_flow_head_backward" in code and "block_sum" in code and "launch_flow_head_backward" in entries
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic", "bf16", "__half"):
        assert word not in code and word not in entries, word
    for word in ("rsqrt", "__frsqrt", "__fdividef", "__fsqrt_r", "__sinf", "__cosf", "__expf"):      # IEEE sqrt / division, double sin / cos
        assert word not in code, word
    assert code.count("hipLaunchKernelGGL") == 2       # one launch per direction
    py = open(os.path.join(ROOT, "splatfields_amd", "flow_head.py")).read()
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in py, word


def test_path_selection_order():
    """keyword > set_flow_head > SPLATFIELDS_FLOW_HEAD > "torch"; the keyword also arrives through SplatFields / hyper_args"""
    import splatfields_amd
    from splatfields_amd import flow_head as fh
    from splatfields_amd.deform_field import FlowHead, SplatFields, SplatFieldsModel
    assert os.environ.get("SPLATFIELDS_FLOW_HEAD") or fh.flow_head_path() == "torch"
    prev = splatfields_amd.set_flow_head("fused")
    try:
        assert fh.flow_head_path() == "fused" and fh.resolve_flow_head(None) == "fused" and fh.resolve_flow_head("torch") == "torch"
        assert splatfields_amd.set_flow_head("torch") == "fused" and fh.resolve_flow_head(None) == "torch" and fh.resolve_flow_head("fused") == "fused"
        with pytest.raises(ValueError, match="unknown flow-head path"):
            splatfields_amd.set_flow_head("hip")
        assert fh.flow_head_path() == "torch"
    finally:
        splatfields_amd.set_flow_head(prev)
    with pytest.raises(ValueError, match="unknown flow-head path"):
        FlowHead(W=32, flow_model="se3", path="hip")
    quick = dict(encoder_type="none", deform_d=2, rgb_d=2, flow_d=2, scale_d=2, opacity_d=2, rotation_d=2)
    assert SplatFields(n_frames=3, **quick).mlp_flow_head.path is None
    assert SplatFields(n_frames=3, flow_head="fused", **quick).mlp_flow_head.path == "fused"
    import types
    model = SplatFieldsModel(types.SimpleNamespace(n_frames=3, flow_head="fused", flow_model="se3Scaled", **quick), device="cpu")
    assert model.deform.mlp_flow_head.path == "fused" and model.deform.mlp_flow_head.flow_model == "se3Scaled"
    # the state dict does not know the path
    a, b = (FlowHead(W=32, flow_model="dct_siren", path=pth) for pth in ("torch", "fused"))
    assert list(a.state_dict()) == list(b.state_dict())
    # the environment variable is the process default, read at import
    code = "import splatfields_amd.flow_head as f; print(f.flow_head_path(), f.resolve_flow_head(None), f.resolve_flow_head('torch'))"
    for value, want in (("fused", "fused fused torch"), ("", "torch torch torch")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_FLOW_HEAD=value), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr)
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_FLOW_HEAD="hip"), capture_output=True, text=True)
    assert bad.returncode != 0 and "unknown flow-head path" in bad.stderr


def test_unsupported_shapes_are_refused_at_construction_and_cpu_tensors_at_the_call():
    from splatfields_amd.deform_field import FlowHead
    from splatfields_amd.flow_head import fused_flow_head
    for kw in (dict(W=130), dict(W=260), dict(W=2), dict(W=128, flow_model="dct", num_basis=11), dict(W=128, flow_model="dct_siren", num_basis=0)):
        args = dict(dict(flow_model="se3", n_frames=6), **kw)
        with pytest.raises(ValueError, match="fused"):
            FlowHead(path="fused", **args)
        if args.get("num_basis", 4) > 0:
            FlowHead(path="torch", **args)          # the PyTorch-op path has no such limit
            FlowHead(**args)
    head = FlowHead(W=32, flow_model="se3", path="fused")
    with pytest.raises(RuntimeError, match="no CPU path"):
        head(torch.randn(5, 32), torch.randn(5, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_flow_head("offset", torch.randn(5, 32), torch.randn(5, 3), [torch.randn(3, 32)], [torch.randn(3)])
