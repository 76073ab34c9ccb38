"""The C ABI of the evaluation metrics (include/splatraster.h: sr_metrics_workspace_bytes / sr_image_metrics): exported and
bound, its host-only part works without a GPU, and every bad call is refused on the host with a message before any launch."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_metrics_workspace_bytes", "sr_image_metrics")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert "metrics.hip" in build.SOURCES
    assert lib.sr_version() == 4     # additions only: no existing struct or contract changed
    for name, value in (("SR_QUANT_NONE", _lib.QUANT_NONE), ("SR_QUANT_PNG", _lib.QUANT_PNG), ("SR_QUANT_TO8B", _lib.QUANT_TO8B)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    import splatfields_amd
    for name in ("image_metrics", "compute_psnr", "compute_ssim", "psnr"):
        assert callable(getattr(splatfields_amd, name)), name


def test_workspace_follows_the_tiles_of_the_valid_map(lib):
    ws = lib.sr_metrics_workspace_bytes
    tiles = lambda h, w: -(-(h - 10) // 32) * -(-(w - 10) // 32)
    for b, h, w in ((1, 11, 11), (1, 42, 42), (1, 43, 42), (1, 600, 800), (1, 800, 800), (8, 800, 800), (3, 1600, 1600)):
        need = 2 * 8 * 3 * b * tiles(h, w)                     # two double partial sums per 32 x 32 tile of every plane
        assert ws(b, h, w) % 256 == 0 and need <= ws(b, h, w) < need + 256, (b, h, w)
    assert ws(1, 42, 42) == ws(1, 11, 11) < ws(1, 800, 800) < ws(8, 800, 800)
    assert ws(1, 43, 75) == ws(1, 74, 106)                      # 2 x 3 tiles either way
    for bad in ((0, 64, 64), (-1, 64, 64), (1, 10, 64), (1, 64, 10), (1, 0, 64), (1, 64, -5), (1 << 20, 1 << 14, 1 << 14)):
        assert ws(*bad) == 0, bad


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch
    chw = lambda h, w: (C.c_longlong * 4)(3 * h * w, h * w, w, 1)

    def call(batch=1, h=16, w=16, pred=p, ps="chw", gt=p, gs="chw", mask=None, mask_item=0, quantize=0, work=p, psnr=p, ssim=p,
             channels=p, frames=None):
        ps = chw(max(h, 1), max(w, 1)) if ps == "chw" else ps
        gs = chw(max(h, 1), max(w, 1)) if gs == "chw" else gs
        return lib.sr_image_metrics(batch, h, w, pred, ps, gt, gs, mask, mask_item, quantize, work, psnr, ssim, channels, frames, None)

    err = lambda: lib.sr_last_error()
    for kw in (dict(batch=0), dict(batch=-2), dict(h=0), dict(w=-1)):
        assert call(**kw) != 0 and b"sizes must be positive" in err(), kw
    for kw in (dict(h=10), dict(w=10), dict(h=1, w=1)):
        assert call(**kw) != 0 and b"height and width >= 11" in err(), kw
    for kw in (dict(pred=None), dict(gt=None), dict(ps=None), dict(gs=None), dict(work=None), dict(psnr=None), dict(ssim=None),
               dict(channels=None)):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    for q in (-1, 3, 255):
        assert call(quantize=q) != 0 and b"unknown quantisation mode" in err(), q
    assert call(frames=p) != 0 and b"need a quantisation mode" in err()
    assert call(batch=1 << 20, h=1 << 14, w=1 << 14) != 0 and b"too large" in err()
    assert call(batch=1 << 30) != 0 and b"too large" in err()
    # a grid holds fewer than 2^32 threads: 6000 x 3 x 31 x 31 workgroups of 256 do not fit, 5000 x 3 x 31 x 31 do
    assert call(batch=6000, h=1002, w=1002) != 0 and b"too large" in err()
    assert lib.sr_metrics_workspace_bytes(6000, 1002, 1002) == 0 < lib.sr_metrics_workspace_bytes(5000, 1002, 1002)
    assert call(ps=(C.c_longlong * 4)(768, 256, -16, 1)) != 0 and b"negative stride" in err()
    assert call(mask=p, mask_item=5) != 0 and b"mask_item_stride" in err()


def test_the_metrics_never_wait_for_the_device_and_have_no_float_atomics():
    from splatfields_amd.build import strip_comments
    text = "\n".join(strip_comments(abi_text.source(f)) for f in ("metrics.hip", "reduce.h", "window11.h"))   # metrics.hip ends with its entry points
    assert "block_sum" in text and "win_filter_column" in text      # the sums and the window it is built from
    assert "sr_image_metrics" in text and "k_metrics" in text and "k_metrics_reduce" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemset", "hipMalloc",
                 "atomicAdd", "atomic"):
        assert word not in text, word
    py = "\n".join(open(os.path.join(ROOT, "splatfields_amd", f)).read() for f in ("metrics.py", "_lib.py"))   # with the shared call helpers
    for word in (".item()", ".cpu()", "synchronize", ".tolist()", ".numpy()"):
        assert word not in py, word


def test_the_kernel_is_specialised_on_mask_and_quantisation():
    text = open(os.path.join(ROOT, "splatfields_amd", "csrc", "metrics.hip")).read()
    assert re.search(r"template <bool kMasked, int kQuant>\s*__global__", text)
    for q in ("SR_QUANT_NONE", "SR_QUANT_PNG", "SR_QUANT_TO8B"):
        assert "k_metrics<kMasked, %s>" % q in text, q
    assert "launch_metrics_quant<true>" in text and "launch_metrics_quant<false>" in text
