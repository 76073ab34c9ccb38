"""The C ABI of LPIPS (include/splatraster.h: sr_lpips_*): declared, exported and bound with the header's signatures, SR_VERSION
still 4, the sizes the library reports, every bad call refused on the host with a message before anything is launched, and the
conditions the op shares with the other fused ops (no atomics, no host wait, the shared fixed-order sums)."""
import ctypes as C
import re

import pytest

import abi_text
from test_c_abi import bound_as

NAMES = ("sr_lpips_packed_bytes", "sr_lpips_pack_weights", "sr_lpips_workspace_bytes", "sr_lpips_maps_floats", "sr_lpips_forward")
CONVS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512), (512, 512),
         (512, 512), (512, 512))
TAPS = (64, 128, 256, 512, 512)


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_and_bound(lib):
    from splatfields_amd import _lib, build
    protos = abi_text.prototypes()
    for name in NAMES:
        assert name in protos and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert abi_text.entry_point(name)                                  # defined once, in one of build.SOURCES
        assert name in abi_text.source("lpips.hip"), name
        ret, args = protos[name]
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype in bound_as(ret)[:1] and len(argtypes) == len(args), name
        for arg, ctype in zip(args, argtypes):
            assert ctype in bound_as(arg), (name, arg, ctype)
    assert "lpips.hip" in build.SOURCES and "quantise.h" in build.HEADERS and "reduce.h" in build.HEADERS
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define\s+SR_VERSION\s+4\b", abi_text.header())
    d = abi_text.defines()
    assert (int(d["SR_LPIPS_CONVS"]), int(d["SR_LPIPS_TAPS"])) == (_lib.LPIPS_CONVS, _lib.LPIPS_TAPS) == (13, 5)


def test_python_and_kernel_agree_on_the_network():
    from splatfields_amd import lpips
    assert lpips.CONV_CHANNELS == CONVS and lpips.TAP_CHANNELS == TAPS and lpips.MIN_SIDE == 16
    text = abi_text.source("lpips.hip")
    assert "kLpCin[kLpLayers] = {%s}" % ", ".join(str(c) for c, _ in CONVS) in text
    assert "kLpCout[kLpLayers] = {%s}" % ", ".join(str(c) for _, c in CONVS) in text
    assert "kLpTapC[kLpTaps] = {%s}" % ", ".join(map(str, TAPS)) in text
    assert "kLpLaunches = %d" % lpips.LAUNCHES_PER_CHUNK in text and lpips.LAUNCHES_PER_CHUNK == 19


def test_sizes(lib):
    up = lambda v: (v + 255) // 256 * 256
    floats = sum(up(4 * 9 * ci * co) for ci, co in CONVS) + sum(up(4 * co) for _, co in CONVS) + sum(up(4 * c) for c in TAPS) + 2 * 256
    assert lib.sr_lpips_packed_bytes() == floats
    for b, h, w in ((1, 16, 16), (4, 37, 53), (3, 64, 48), (8, 800, 800)):
        act, pool = 4 * 2 * b * h * w * 64, 4 * 2 * b * (h // 2) * (w // 2) * 64
        partial = 8 * b * sum(((h >> l) * (w >> l) + 63) // 64 for l in range(5))
        assert lib.sr_lpips_workspace_bytes(b, h, w) == 2 * up(act) + up(pool) + up(partial), (b, h, w)
        assert lib.sr_lpips_maps_floats(b, h, w) == b * sum((h >> l) * (w >> l) for l in range(5))
    assert lib.sr_lpips_workspace_bytes(8, 800, 800) > 4 << 30                  # byte offsets are 64-bit
    for b, h, w in ((0, 16, 16), (1, 15, 16), (1, 16, 15), (1, 32769, 16), (1 << 20, 4096, 4096)):
        assert lib.sr_lpips_workspace_bytes(b, h, w) == 0 and lib.sr_lpips_maps_floats(b, h, w) == 0, (b, h, w)
    # 2 batch x tiles of 8 x 16 pixels must fit a grid of 2^31 - 1 workgroups: 32768 x 32768 has 2^23 tiles
    assert lib.sr_lpips_workspace_bytes(127, 32768, 32768) > 0 and lib.sr_lpips_workspace_bytes(128, 32768, 32768) == 0


def test_bad_calls_are_refused_on_the_host(lib):
    buf = (C.c_double * 1024)()
    base = C.addressof(buf)
    base += (-base) % 256
    p = C.c_void_p(base)
    strides = (C.c_longlong * 4)(768, 256, 16, 1)
    err = lambda: lib.sr_last_error()

    def call(batch=1, h=16, w=16, pred=p, ps=strides, gt=p, gs=strides, quantize=0, packed=p, work=p, out=p, taps=None, maps=None):
        return lib.sr_lpips_forward(batch, h, w, pred, ps, gt, gs, quantize, packed, work, out, taps, maps, None)

    assert call(batch=0) != 0 and b"sizes must be positive" in err()
    assert call(h=15) != 0 and b"relu5_3 has no pixel" in err()
    assert call(w=15) != 0 and b"relu5_3 has no pixel" in err()
    assert call(h=32769) != 0 and b"too large" in err()
    assert call(batch=128, h=32768, w=32768) != 0 and b"too large" in err()
    for kw in (dict(pred=None), dict(gt=None), dict(ps=None), dict(gs=None), dict(packed=None), dict(out=None)):
        assert call(**kw) != 0 and b"null pointer in sr_lpips_forward" in err(), kw
    assert call(work=None) != 0 and b"null or misaligned workspace" in err()
    assert call(work=C.c_void_p(base + 16)) != 0 and b"null or misaligned workspace" in err()
    assert call(packed=C.c_void_p(base + 16)) != 0 and b"misaligned blob" in err()
    assert call(out=C.c_void_p(base + 2)) != 0 and b"misaligned pointer" in err()
    assert call(quantize=3) != 0 and b"unknown quantisation mode" in err()
    assert call(ps=(C.c_longlong * 4)(768, 256, -16, 1)) != 0 and b"negative stride" in err()

    table = (C.c_void_p * 13)(*([base] * 13))
    lins = (C.c_void_p * 5)(*([base] * 5))
    pack = lambda cw=table, cb=table, ls=lins, shift=p, scale=p, packed=p: lib.sr_lpips_pack_weights(cw, cb, ls, shift, scale, packed, None)
    for kw in (dict(cw=None), dict(cb=None), dict(ls=None), dict(shift=None), dict(scale=None), dict(packed=None)):
        assert pack(**kw) != 0 and b"null pointer in sr_lpips_pack_weights" in err(), kw
    holes = (C.c_void_p * 13)(*([base] * 7 + [None] + [base] * 5))
    assert pack(cw=holes) != 0 and b"convolution 7" in err()
    assert pack(ls=(C.c_void_p * 5)(base, base, None, base, base)) != 0 and b"lin 2" in err()
    assert pack(packed=C.c_void_p(base + 64)) != 0 and b"misaligned blob" in err()


def test_the_op_keeps_the_conditions_of_the_fused_ops():
    import os
    from splatfields_amd.build import strip_comments
    text = strip_comments(abi_text.source("lpips.hip"))
    assert "block_sum" in text and "wave_sum" in text and '#include "reduce.h"' in text      # the shared fixed-order sums
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in text and "bf16" not in text              # exact f32-input MFMA only
    assert "quantise<kQuant>" in text and '#include "quantise.h"' in text                     # the quantisation of image_metrics, shared
    for word in ("hipDeviceSynchronize", "hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemset", "hipMalloc", "atomic",
                 "asm"):
        assert word not in text, word
    assert text.count("hipLaunchKernelGGL") >= 6
    py = open(os.path.join(abi_text.ROOT, "splatfields_amd", "lpips.py")).read()
    for word in (".item()", ".cpu()", "synchronize", ".tolist()", ".numpy()"):
        assert word not in py, word
    assert "quantise<kQuant>" in strip_comments(abi_text.source("metrics.hip")) and "float quantise(" not in abi_text.source("metrics.hip")


def test_header_names_the_reference_range():
    import os
    text = open(os.path.join(abi_text.ROOT, "include", "splatraster.h")).read()
    block = text[text.index("Which upstream interface each entry replaces"):text.index("Conventions (SURVEY.md Appendix A)")]
    at = block.index("sr_lpips_pack_weights + sr_lpips_forward")
    assert "render.py:174-180" in block[at:at + 400] and "render.py:163-207" in block[at:at + 400]
