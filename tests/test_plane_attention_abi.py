"""The C ABI of the plane generator's attention kernels (include/splatraster.h: sr_attention_*): exported and bound with the
header's signatures, the size queries work without a GPU, every bad call is refused on the host before any launch with a message
that names the cause, the ABI version stays 4; and the Python switches (attention= / set_attention /
SPLATFIELDS_PLANE_ATTENTION / config["attention"] / encoder_args["attention"]) resolve as documented."""
import ctypes as C
import importlib.util
import os
import re

import pytest

import abi_text
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sr_attention_saved_bytes", "sr_attention_backward_workspace", "sr_attention_forward", "sr_attention_backward")


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_exported_with_the_headers_signatures(lib):
    from splatfields_amd import _lib, build
    header = abi_text.header()
    for name in NAMES:                  # the signatures: test_c_abi.py::test_every_prototype_matches_the_binding
        assert name in abi_text.prototypes() and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "attention.hip" in build.SOURCES
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define SR_VERSION 4\b", header)


def test_job_struct_matches_the_header():
    from splatfields_amd import _lib
    fields = [f[1] for f in abi_text.structs()["SrAttentionJob"]]      # in the binding's order: test_c_abi.py
    assert C.sizeof(_lib.SrAttentionJob) == 8 * len(fields)
    wanted = {"x", "gamma", "beta", "stats", "out", "saved", "dy", "dx"}
    assert wanted <= set(fields) and len(fields) == len(wanted) + 8 + 10       # + the eight projection tensors + ten parameter gradients
    # the plane generator's own row is unchanged
    assert [n for n, _ in _lib.SrPlaneJob._fields_] == ["x", "weight", "bias", "gamma", "beta", "stats", "residual", "out", "pre", "dy", "dx", "dweight",
                                                       "dbias", "dgamma", "dbeta", "d_residual", "add", "dx_out"]


def test_size_queries_are_monotone_and_zero_for_unsupported_shapes(lib):
    queries = (lib.sr_attention_saved_bytes, lib.sr_attention_backward_workspace)
    sizes = ((1, 2), (3, 5), (5, 13), (9, 9), (20, 20), (32, 32), (33, 32), (64, 64))
    for q in queries:
        for n0, n1 in ((1, 2), (2, 3), (3, 8)):
            for h, w in sizes:
                assert 0 < q(n0, 32, 32, h, w) < q(n1, 32, 32, h, w)
        got = [q(3, 32, 4, h, w) for h, w in sizes]                     # with the tokens
        assert got == sorted(got) and len(set(got)) == len(got), got
        got = [q(3, c, 1, 20, 20) for c in (8, 16, 24, 32, 48, 64)]     # with the channels
        assert got == sorted(got) and len(set(got)) == len(got), got
        assert q(3, 32, 4, 20, 20) % 8 == 0 and q(3, 32, 4, 20, 20) % 3 == 0      # equal pieces of doubles, one per plane
        for bad in ((0, 32, 4, 20, 20), (-1, 32, 4, 20, 20), (9, 32, 4, 20, 20), (3, 0, 1, 20, 20), (3, 12, 4, 20, 20), (3, 72, 4, 20, 20),
                    (3, 32, 5, 20, 20), (3, 32, 0, 20, 20), (3, 32, 4, 0, 20), (3, 32, 4, 20, 0), (3, 32, 4, 4097, 1), (3, 32, 4, 64, 65),
                    (3, 32, 32, 1, 1), (3, 8, 8, 1, 1)):
            assert q(*bad) == 0, bad
        assert q(3, 32, 4, 64, 64) > 0 and q(3, 32, 4, 1, 1) > 0 and q(8, 64, 64, 1, 2) > 0


def test_bad_calls_are_refused_on_the_host(lib):
    from splatfields_amd import _lib
    buf = (C.c_float * 1024)()
    p = C.addressof(buf)               # host memory: never dereferenced, every check comes before the launch
    jobs = (_lib.SrAttentionJob * 3)()
    for j in jobs:
        for name, _ in _lib.SrAttentionJob._fields_:
            setattr(j, name, p)
    ws = C.c_void_p(p)
    err = lambda: lib.sr_last_error()

    def fwd(n=3, jobs=jobs, c=32, groups=4, h=4, w=4, ws=None):
        return lib.sr_attention_forward(n, jobs, c, groups, h, w, 1e-6, None)

    def bwd(n=3, jobs=jobs, c=32, groups=4, h=4, w=4, ws=ws):
        return lib.sr_attention_backward(n, jobs, c, groups, h, w, 1e-6, ws, None)

    for fn in (fwd, bwd):
        for n in (0, -1, 9):
            assert fn(n=n) != 0 and b"n_planes" in err(), (fn.__name__, n)
        for c in (0, 12, 72):
            assert fn(c=c) != 0 and b"multiple of 8 in 8..64" in err(), (fn.__name__, c)
        for g in (0, 3, 5, 64):
            assert fn(groups=g) != 0 and b"groups must divide channels" in err(), (fn.__name__, g)
        for kw in (dict(h=0), dict(w=0), dict(h=4097, w=1), dict(h=64, w=65), dict(h=-4, w=-4)):
            assert fn(**kw) != 0 and b"1..4096 tokens" in err(), (fn.__name__, kw)
        for kw in (dict(c=32, groups=32, h=1, w=1), dict(c=8, groups=8, h=1, w=1)):
            assert fn(**kw) != 0 and b"at least two values" in err(), (fn.__name__, kw)
        assert fn(jobs=None) != 0 and b"null pointer" in err() and b"jobs" in err(), fn.__name__
    assert bwd(ws=None) != 0 and b"null pointer" in err() and b"workspace" in err()
    # a row that lacks a tensor the call needs
    jobs[1].wk = None
    assert fwd() != 0 and b"job 1" in err() and b"sr_attention_forward" in err()
    assert bwd() != 0 and b"job 1" in err() and b"sr_attention_backward" in err()
    jobs[1].wk = p
    jobs[2].saved = None
    assert fwd() != 0 and b"job 2" in err()
    assert bwd() != 0 and b"job 2" in err()
    jobs[2].saved = p
    jobs[0].dbk = None
    assert bwd() != 0 and b"job 0" in err()
    jobs[0].dbk, jobs[0].out = p, None
    assert fwd() != 0 and b"job 0" in err()


# ---- the selection API ------------------------------------------------------------------------------------------------------
def test_process_default_setter_and_keywords():
    import splatfields_amd
    from splatfields_amd import plane_generator as pg
    start = pg.attention()
    try:
        assert splatfields_amd.set_attention("fused") == start and pg.attention() == "fused"
        assert pg.resolve_attention(None) == "fused" and pg.resolve_attention("torch") == "torch"
        assert pg.set_attention("torch") == "fused" and pg.resolve_attention(None) == "torch"
        with pytest.raises(ValueError, match="unknown plane-generator attention"):
            pg.set_attention("flash")
        assert pg.attention() == "torch"                                            # a refused name changes nothing
    finally:
        pg.set_attention(start)
    small = dict(in_channels=8, out_channels=16, up_block_types=("TimeUpDecoderBlock2D",), block_out_channels=(16,), norm_num_groups=4, layers_per_block=1)
    net = pg.TimeVAEDecoder(**small)
    assert net.attention is None and pg.TimeVAEDecoder(**small, attention="fused").attention == "fused"
    assert set(pg.TimeVAEDecoder(**small, attention="fused").state_dict()) == set(net.state_dict())     # not part of the state dict
    with pytest.raises(ValueError, match="unknown plane-generator attention"):
        pg.TimeVAEDecoder(**small, attention="sdpa")
    assert pg.Tensorial2D(8, 16, 2, attention="fused").net.attention == "fused" and pg.Tensorial2D(8, 16, 2).net.attention is None
    enc = pg.VarTriPlaneEncoder({"noise_res": 2, "attention": "fused"})
    assert all(s.net.attention == "fused" for s in enc.subs)
    assert all(s.net.attention is None for s in pg.VarTriPlaneEncoder({"noise_res": 2}).subs)
    with pytest.raises(ValueError, match="unknown plane-generator attention"):
        pg.generate_planes([net], [torch.zeros(1, 8, 2, 2)], attention="sdpa")
    assert pg.ATTENTION_LAUNCHES[0] <= 4 and pg.ATTENTION_LAUNCHES[1] <= 8
    # there is no CPU path, and unsupported shapes are refused before anything is launched
    with pytest.raises(RuntimeError, match="no CPU path"):
        pg.fused_attention(*[[torch.zeros(s)] for s in ((8, 2, 2), (8,), (8,)) + ((8, 8), (8,)) * 4], groups=1)
    with pytest.raises(ValueError, match="one tensor per plane"):
        pg.fused_attention([torch.zeros(8, 2, 2)] * 2, *[[torch.zeros(8)]] * 10)


def test_environment_variable_sets_the_initial_default(monkeypatch):
    """SPLATFIELDS_PLANE_ATTENTION is read once, when the module is first imported: a second copy of the module is imported here
    under another name, the package's own copy is not touched"""
    path = os.path.join(ROOT, "splatfields_amd", "plane_generator.py")

    def fresh(value):
        if value is None:
            monkeypatch.delenv("SPLATFIELDS_PLANE_ATTENTION", raising=False)
        else:
            monkeypatch.setenv("SPLATFIELDS_PLANE_ATTENTION", value)
        spec = importlib.util.spec_from_file_location("splatfields_amd._plane_generator_env_probe", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    assert fresh(None).attention() == "torch" and fresh("").attention() == "torch"
    assert fresh("torch").attention() == "torch" and fresh("fused").attention() == "fused"
    with pytest.raises(ValueError, match="unknown plane-generator attention"):
        fresh("flash")


def test_splatfields_accepts_the_attention_key():
    from splatfields_amd.deform_field import SplatFields
    small = dict(deform_w=64, deform_d=2, deform_skips=[1], rgb_w=64, rgb_d=2, rgb_skips=[0], flow_w=64, flow_d=2, flow_skips=[1],
                 scale_d=2, scale_skips=[0], opacity_d=2, opacity_skips=[5], rotation_d=2)
    model = SplatFields(encoder_args={"generator": "decoder", "noise_res": 2, "attention": "fused"}, n_frames=0, **small)
    assert all(s.net.attention == "fused" for s in model.encoder.subs)
    plain = SplatFields(encoder_args={"generator": "decoder", "noise_res": 2}, n_frames=0, **small)
    assert all(s.net.attention is None for s in plain.encoder.subs)
    assert set(model.state_dict()) == set(plain.state_dict())
    with pytest.raises(ValueError, match="not arguments of the plane generator"):
        SplatFields(encoder_args={"generator": "decoder", "noise_res": 2, "attn": "fused"}, n_frames=0, **small)
    with pytest.raises(ValueError, match="unknown plane-generator attention"):
        SplatFields(encoder_args={"generator": "decoder", "noise_res": 2, "attention": "flash"}, n_frames=0, **small)
