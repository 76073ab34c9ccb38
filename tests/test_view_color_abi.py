"""The C ABI of the fused view-dependent colour head (include/splatraster.h: sr_view_color_*): declared, exported and bound with
matching signatures and constants, additions only, every bad call refused on the host with a message before any launch, and
the selection of the path (keyword > set_view_color > SPLATFIELDS_VIEW_COLOR > "torch")."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_view_color_saved_bytes", "sr_view_color_workspace_bytes", "sr_view_color_forward", "sr_view_color_backward")
CAMERAS, DIRS = 0, 1


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound_with_matching_signatures(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    assert "view_color.hip" in build.SOURCES and "point_tile.h" in build.HEADERS
    for name in NEW:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define SR_VERSION 4\b", header)      # functions are added, none changes
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(SR_VIEW_[A-Z0-9_]+)\s+(\d+)\b", header, re.M)}
    assert defs == {"SR_VIEW_FROM_CAMERAS": _lib.VIEW_FROM_CAMERAS, "SR_VIEW_DIRS_GIVEN": _lib.VIEW_DIRS_GIVEN,
                    "SR_VIEW_MAX_WIDTH": _lib.VIEW_MAX_WIDTH, "SR_VIEW_MAX_VIEWS": _lib.VIEW_MAX_VIEWS}
    assert (_lib.VIEW_FROM_CAMERAS, _lib.VIEW_DIRS_GIVEN, _lib.VIEW_MAX_WIDTH, _lib.VIEW_MAX_VIEWS) == (CAMERAS, DIRS, 256, 16)
    import splatfields_amd
    for name in ("set_view_color", "view_color_path", "fused_view_color"):
        assert callable(getattr(splatfields_amd, name)), name
    from splatfields_amd import view_color
    assert view_color.VIEW_COLORS == ("torch", "fused") and view_color.VIEW_COLOR_LAUNCHES == (1, 3)


def test_size_queries_and_the_restated_limits(lib):
    from splatfields_amd import _lib
    for n in (1, 1000, 300_000):
        for v in (1, 16):
            assert lib.sr_view_color_saved_bytes(n, 128, v) >= 3 * 8 * n and lib.sr_view_color_saved_bytes(n, 128, v) % 256 == 0
            assert lib.sr_view_color_workspace_bytes(n, 128, v) >= (n + 255) // 256 * 12 * 8
    for query in (lib.sr_view_color_saved_bytes, lib.sr_view_color_workspace_bytes):
        assert query(0, 128, 1) > 0                                       # an empty call is supported
        for bad in ((100, 130, 1), (100, 0, 1), (100, 260, 1), (100, -4, 1), (100, 2, 1), (-1, 128, 1), (1 << 31, 128, 1), (100, 128, 0),
                    (100, 128, 17), (100, 128, -1)):
            assert query(*bad) == 0, bad
        assert query(100, 256, 16) > 0 and query(100, 4, 1) > 0 and query((1 << 31) - 1, 128, 1) > 0
    # the Python restatement refuses exactly what the library refuses
    for width in (-4, 0, 2, 4, 36, 128, 130, 256, 260):
        for n_views in (-1, 0, 1, 16, 17):
            assert (_lib.view_color_shape_error(width, n_views) is None) == (lib.sr_view_color_saved_bytes(100, width, n_views) > 0), (width, n_views)
    assert "multiple of 4" in _lib.view_color_shape_error(130, 1) and "views" in _lib.view_color_shape_error(128, 17)


def test_bad_calls_are_refused_on_the_host_and_empty_ones_launch_nothing(lib):
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    p, odd8, odd4, odd2 = C.c_void_p(base), C.c_void_p(base + 8), C.c_void_p(base + 4), C.c_void_p(base + 2)      # host memory: never dereferenced
    err = lambda: lib.sr_last_error()

    def fwd(mode=CAMERAS, n=10, width=128, v=3, feature=p, means=p, cams=p, weight=p, bias=p, colours=p, saved=p):
        return lib.sr_view_color_forward(mode, n, width, v, feature, means, cams, weight, bias, colours, saved, None)

    def bwd(mode=CAMERAS, n=10, width=128, v=3, means=p, cams=p, weight=p, saved=p, g=p, d_feature=p, d_pos=p, dz=p, ws=p):
        return lib.sr_view_color_backward(mode, n, width, v, means, cams, weight, saved, g, d_feature, d_pos, dz, ws, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(width=130), b"multiple of 4"), (dict(width=260), b"multiple of 4"), (dict(width=0), b"multiple of 4"),
                        (dict(width=2), b"multiple of 4"), (dict(v=0), b"n_views"), (dict(v=17), b"n_views"), (dict(v=-3), b"n_views"),
                        (dict(mode=2), b"unknown mode"), (dict(mode=-1), b"unknown mode"), (dict(n=-1), b"n_points"), (dict(n=1 << 31), b"n_points"),
                        (dict(cams=None), b"null pointer"), (dict(weight=None), b"null pointer"), (dict(means=None), b"reads means3D"),
                        (dict(weight=odd4), b"16-byte aligned"), (dict(weight=odd8), b"16-byte aligned"), (dict(cams=odd2), b"aligned"),
                        (dict(means=odd2), b"aligned"), (dict(saved=odd4), b"aligned")):
            assert call(**kw) != 0 and msg in err(), (call.__name__, kw, err())
        assert call(n=0, cams=None, weight=None, means=None, saved=None) == 0            # no points: valid, nothing is launched
        assert call(n=0, width=130) != 0 and call(n=0, v=17) != 0                         # but the shape is still checked
    for kw, msg in ((dict(feature=None), b"null pointer"), (dict(bias=None), b"null pointer"), (dict(colours=None), b"null pointer"),
                    (dict(feature=odd4), b"16-byte aligned"), (dict(feature=odd8), b"16-byte aligned"), (dict(colours=odd2), b"aligned"),
                    (dict(bias=odd2), b"aligned")):
        assert fwd(**kw) != 0 and msg in err(), (kw, err())
    for kw, msg in ((dict(saved=None), b"null pointer"), (dict(g=None), b"null pointer"), (dict(dz=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(dz=odd4), b"16-byte aligned"), (dict(dz=odd8), b"16-byte aligned"), (dict(d_feature=odd4), b"16-byte aligned"),
                    (dict(ws=odd4), b"aligned"), (dict(g=odd2), b"aligned"), (dict(d_pos=odd2), b"aligned")):
        assert bwd(**kw) != 0 and msg in err(), (kw, err())


def test_nothing_waits_for_the_device_and_nothing_is_added_atomically():
    from splatfields_amd.build import strip_comments
    code = strip_comments(abi_text.source("view_color.hip")) + strip_comments(abi_text.source("point_tile.h"))
    entries = "\n".join(abi_text.entry_point(name) for name in NEW)
    assert "k_view_color_forward" in code and "k_view_color_backward" in code and "block_sum" in code and "launch_view_color_backward" in entries
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMalloc", "atomic", "bf16", "__half"):
        assert word not in code and word not in entries, word
    for word in ("rsqrt", "__frsqrt", "__fdividef", "__fsqrt_r", "__expf", "expf("):      # IEEE sqrt / division, the double exp
        assert word not in code, word
    assert code.count("hipLaunchKernelGGL") == 2       # one launch per direction
    py = open(os.path.join(ROOT, "splatfields_amd", "view_color.py")).read()
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in py, word


def test_path_selection_order(monkeypatch):
    """keyword > set_view_color > SPLATFIELDS_VIEW_COLOR > "torch"; the keyword also arrives through SplatFields / hyper_args"""
    import types
    import splatfields_amd
    from splatfields_amd import general_mlp, view_color as vc
    from test_general_mlp import formula
    monkeypatch.setattr(general_mlp, "fused_general_mlp", formula)      # the networks run on CPU tensors here
    from splatfields_amd.deform_field import SplatFields, SplatFieldsModel
    assert os.environ.get("SPLATFIELDS_VIEW_COLOR") or vc.view_color_path() == "torch"
    quick = dict(encoder_type="none", deform_d=2, rgb_d=2, scale_d=2, opacity_d=2, rotation_d=2, deform_skips=[0], rgb_skips=[0], scale_skips=[0],
                 opacity_skips=[0], rgb_w=64, use_view_dep_rgb=True)
    free, pinned = SplatFields(n_frames=0, **quick), SplatFields(n_frames=0, view_color="torch", **quick)
    assert free.view_color is None and pinned.view_color == "torch" and SplatFields(n_frames=0, view_color="fused", **quick).view_color == "fused"
    x, t = torch.rand(4, 3), torch.zeros(4, 1)
    prev = splatfields_amd.set_view_color("fused")
    try:
        assert vc.view_color_path() == "fused" and vc.resolve_view_color(None) == "fused" and vc.resolve_view_color("torch") == "torch"
        assert free(x, t)["rgb_fnc"].path == "fused" and pinned(x, t)["rgb_fnc"].path == "torch"      # resolved at call time
        assert splatfields_amd.set_view_color("torch") == "fused" and vc.resolve_view_color(None) == "torch" and vc.resolve_view_color("fused") == "fused"
        with pytest.raises(ValueError, match="unknown view-colour path"):
            splatfields_amd.set_view_color("hip")
        assert vc.view_color_path() == "torch"
    finally:
        splatfields_amd.set_view_color(prev)
    with pytest.raises(ValueError, match="unknown view-colour path"):
        SplatFields(n_frames=0, view_color="hip", **quick)
    model = SplatFieldsModel(types.SimpleNamespace(n_frames=0, view_color="fused", **quick), device="cpu")
    assert model.deform.view_color == "fused"
    # the state dict does not know the path
    assert list(free.state_dict()) == list(model.deform.state_dict()) and "mlp_rgb_viewdep.0.weight" in free.state_dict()
    # the environment variable is the process default, read at import
    code = "import splatfields_amd.view_color as f; print(f.view_color_path(), f.resolve_view_color(None), f.resolve_view_color('torch'))"
    for value, want in (("fused", "fused fused torch"), ("", "torch torch torch")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_VIEW_COLOR=value), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == want, (value, out.stdout, out.stderr)
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPLATFIELDS_VIEW_COLOR="hip"), capture_output=True, text=True)
    assert bad.returncode != 0 and "unknown view-colour path" in bad.stderr
