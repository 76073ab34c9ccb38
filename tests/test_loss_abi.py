"""The C ABI of the fused photometric loss (include/splatraster.h: sr_loss_* / sr_photometric_*): exported and bound, its
host-only parts work without a GPU, and every bad call is refused on the host with a message before any launch."""
import ctypes as C
import os
import re

import pytest

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_loss_workspace_bytes", "sr_loss_maps_bytes", "sr_photometric_forward", "sr_photometric_backward")


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
    assert "loss.hip" in build.SOURCES
    assert lib.sr_version() == 4     # additions only: no existing struct or contract changed


def test_workspace_grows_with_the_image_and_is_256_byte_granular(lib):
    sizes = [lib.sr_loss_workspace_bytes(3, h, w) for h, w in ((1, 1), (64, 64), (600, 800), (800, 800), (1600, 1600))]
    assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[3] < sizes[4]
    assert lib.sr_loss_workspace_bytes(6, 800, 800) > lib.sr_loss_workspace_bytes(3, 800, 800)
    assert lib.sr_loss_workspace_bytes(3, 800, 800) >= 3 * 4 * 3 * 25 * 25        # three partial sums per 32 x 32 tile
    assert lib.sr_loss_maps_bytes(3, 800, 800) >= 3 * 3 * 800 * 800 * 4 and lib.sr_loss_maps_bytes(3, 800, 800) % 256 == 0
    for bad in ((0, 8, 8), (3, 0, 8), (3, 8, -1)):
        assert lib.sr_loss_workspace_bytes(*bad) == 0 and lib.sr_loss_maps_bytes(*bad) == 0


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_float * 1024)()
    p = C.c_void_p(C.addressof(buf))       # host memory: never dereferenced, every check comes before the launch

    def fwd(batch=1, channels=3, h=8, w=8, image=p, gt=p, alpha=None, mask=None, lam=0.2, lam_mask=0.0, work=p, maps=None,
            loss=p, l1=p, ssim=p, mask_l1=None):
        return lib.sr_photometric_forward(batch, channels, h, w, image, gt, alpha, mask, lam, lam_mask, work, maps, loss, l1, ssim,
                                          mask_l1, None)

    def bwd(batch=1, channels=3, h=8, w=8, image=p, gt=p, alpha=None, mask=None, maps=p, w_l1=0.8, w_ssim=-0.2, w_mask=0.0, g=p,
            per_item=0, d_image=p, d_alpha=None):
        return lib.sr_photometric_backward(batch, channels, h, w, image, gt, alpha, mask, maps, w_l1, w_ssim, w_mask, g, per_item,
                                           d_image, d_alpha, None)

    err = lambda: lib.sr_last_error()
    for kw in (dict(batch=0), dict(channels=-1), dict(h=0), dict(w=0)):
        assert fwd(**kw) != 0 and b"sizes must be positive" in err(), kw
        assert bwd(**kw) != 0 and b"sizes must be positive" in err(), kw
    for kw in (dict(image=None), dict(gt=None), dict(work=None), dict(loss=None), dict(l1=None)):
        assert fwd(**kw) != 0 and b"null pointer" in err(), kw
    for kw in (dict(image=None), dict(gt=None), dict(g=None), dict(d_image=None)):
        assert bwd(**kw) != 0 and b"null pointer" in err(), kw
    for kw in (dict(alpha=p), dict(mask=p)):
        assert fwd(**kw) != 0 and b"both or neither" in err(), kw
        assert bwd(**kw) != 0 and b"both or neither" in err(), kw
    assert fwd(alpha=p, mask=p) != 0 and b"mask_l1" in err()
    assert fwd(lam_mask=0.1) != 0 and b"lambda_mask without alpha" in err()
    assert fwd(ssim=None) != 0 and b"ssim output may be omitted only" in err()
    assert bwd(maps=None) != 0 and b"needs the maps" in err()
    assert bwd(d_alpha=p) != 0 and b"dL_dalpha without alpha" in err()
    assert fwd(batch=1 << 20, channels=1 << 20) != 0 and b"too large" in err()


def test_the_loss_never_waits_for_the_device_and_has_no_float_atomics():
    from splatfields_amd.build import strip_comments
    text = "\n".join(strip_comments(abi_text.source(f)) for f in ("loss.hip", "reduce.h", "window11.h"))   # loss.hip ends with its entry points
    assert "block_sum" in text and "win_filter_column" in text      # the sums and the window it is built from
    assert "sr_photometric_backward" in text and "k_loss_forward" in text
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy(", "hipMemcpyAsync", "atomicAdd",
                 "atomic"):
        assert word not in text, word
    py = "\n".join(open(os.path.join(ROOT, "splatfields_amd", f)).read() for f in ("losses.py", "_lib.py"))   # with the shared call helpers
    for word in (".item()", ".cpu()", "synchronize", ".tolist()"):
        assert word not in py, word
