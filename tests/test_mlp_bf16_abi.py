"""The opt-in bf16 precision of the fused MLP chains without a GPU: the two C entry points (include/splatraster.h:
sr_mlp_pack_bf16 / sr_mlp_chain_bf16) are exported, bound and declared with their fp32 siblings' signatures, refuse what those
refuse with the same words, and leave the ABI version alone; the Python switches (precision= / set_mlp_precision /
SPLATFIELDS_MLP_PRECISION / SplatFields(mlp_precision=)) resolve as documented; the host side sizes a bf16 plan's buffer in
bf16.  The kernels themselves: tests/test_gpu_mlp_bf16.py."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_bound_and_additions_only(lib):
    from splatfields_amd import _lib
    header = open(os.path.join(ROOT, "include", "splatraster.h")).read()
    for new, old in (("sr_mlp_pack_bf16", "sr_mlp_pack"), ("sr_mlp_chain_bf16", "sr_mlp_chain")):
        assert hasattr(lib, new) and _lib.SYMBOLS[new] == _lib.SYMBOLS[old]
        decl = lambda name: re.search(r"^int " + name + r"\((.*?)\);", header, re.M).group(1)
        assert decl(new) == decl(old)
    assert decl("sr_mlp_pack_bf16") == "int n_jobs, const SrMlpPackJob* jobs, void* hip_stream"
    assert decl("sr_mlp_chain_bf16") == "int n_points, int hidden_tiles, int n_ops, const SrMlpOp* ops, float negative_slope, void* hip_stream"
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and re.search(r"#define\s+SR_VERSION\s+4\b", header)


def good_op(p, **over):
    from splatfields_amd import _lib
    f = dict(w_packed=p, bias=p, src=p, mask=None, store=p, sign_store=None, mask_bits=None, out_tiles=4, mem_tiles=2, reg_tiles=0,
             src_row=32, epilogue=_lib.MLP_LEAKY, mask_row=0, store_row=64, store_channels=64, store_accumulate=0, keep_state=0)
    f.update(over)
    return _lib.SrMlpOp(**f)


def good_job(p, **over):
    from splatfields_amd import _lib
    f = dict(w=p, bias_src=p, dst=p, bias_dst=p, ld=32, transposed=0, row0=0, n_rows=64, n_mem=20, mem_pad=32, mem_col0=0, n_reg=0,
             reg_width=0, reg_col0=0, out_tiles=4, n_bias=64)
    f.update(over)
    return _lib.SrMlpPackJob(**f)


def test_bad_arguments_are_refused_as_by_the_fp32_entry_points(lib):
    """every check precedes the launch: host memory stands in for device memory and is never dereferenced"""
    from splatfields_amd import _lib
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def both(fn32, fn16, name32, name16, *args):
        r32 = fn32(*args); e32 = lib.sr_last_error()
        r16 = fn16(*args); e16 = lib.sr_last_error()
        assert r32 != 0 and r16 != 0, args
        assert name16.encode() in e16 and e16.replace(name16.encode(), name32.encode()) == e32
        return e16

    def chain(n_points, ht, ops, slope=0.01, n=None, null=False):
        table = (_lib.SrMlpOp * max(len(ops), 1))(*ops)
        return both(lib.sr_mlp_chain, lib.sr_mlp_chain_bf16, "sr_mlp_chain", "sr_mlp_chain_bf16",
                    n_points, ht, len(ops) if n is None else n, None if null else table, slope, None)

    assert b"bad arguments" in chain(-1, 4, [good_op(p)])
    assert b"bad arguments" in chain(10, 4, [good_op(p)], null=True)
    assert b"negative_slope" in chain(10, 4, [good_op(p)], slope=1.0)
    assert b"negative_slope" in chain(10, 4, [good_op(p)], slope=float("nan"))
    for ht, ops in ((5, [good_op(p)]), (4, []), (4, [good_op(p)] * (_lib.MLP_MAX_OPS + 1)), (4, [good_op(p, out_tiles=5)]),
                    (4, [good_op(p, mem_tiles=1)]), (4, [good_op(p, mem_tiles=0)]), (4, [good_op(p, reg_tiles=6)]),
                    (4, [good_op(p, w_packed=None)]), (4, [good_op(p, w_packed=p + 4)]), (4, [good_op(p, bias=p + 4)]),
                    (4, [good_op(p, src=None)]), (4, [good_op(p, src_row=16)]), (4, [good_op(p, epilogue=7)]),
                    (4, [good_op(p, epilogue=_lib.MLP_MASK)]), (4, [good_op(p, store_channels=65)]),
                    (8, [good_op(p), good_op(p, store_channels=0)])):
        assert b"unsupported op list" in chain(10, ht, ops)

    def pack(jobs, n=None, null=False):
        table = (_lib.SrMlpPackJob * max(len(jobs), 1))(*jobs)
        return both(lib.sr_mlp_pack, lib.sr_mlp_pack_bf16, "sr_mlp_pack", "sr_mlp_pack_bf16",
                    len(jobs) if n is None else n, None if null else table, None)

    assert b"bad arguments" in pack([], n=-1)
    assert b"bad arguments" in pack([good_job(p)], null=True)
    for jobs in ([good_job(p)] * (_lib.MLP_MAX_PACK_JOBS + 1), [good_job(p, w=None)], [good_job(p, dst=None)], [good_job(p, dst=p + 8)],
                 [good_job(p, mem_pad=16)], [good_job(p, mem_pad=48)], [good_job(p, reg_width=24)], [good_job(p, n_mem=33)],
                 [good_job(p, n_rows=65)], [good_job(p, out_tiles=0)], [good_job(p, bias_src=None)], [good_job(p, n_bias=65)],
                 [good_job(p), good_job(p, mem_pad=0)]):
        assert b"unsupported job" in pack(jobs)


def test_process_default_setter_and_module_attribute():
    import splatfields_amd
    from splatfields_amd import fused_mlp as fm
    from splatfields_amd.general_mlp import GeneralMLP
    start = splatfields_amd.mlp_precision()
    try:
        assert splatfields_amd.set_mlp_precision("bf16") == start and splatfields_amd.mlp_precision() == "bf16"
        assert fm.resolve_precision(None) == "bf16" and fm.resolve_precision("fp32") == "fp32"
        assert splatfields_amd.set_mlp_precision("fp32") == "bf16" and fm.resolve_precision(None) == "fp32"
        with pytest.raises(ValueError, match="unknown MLP precision"):
            splatfields_amd.set_mlp_precision("fp16")
        assert splatfields_amd.mlp_precision() == "fp32"                       # a refused name changes nothing
    finally:
        splatfields_amd.set_mlp_precision(start)
    kw = dict(in_features=3, out_features=3, hidden_features=64, num_hidden_layers=2, skips=[], multires=2, act="leaky_relu",
              composition_rank=0, n_frames=0)
    net = GeneralMLP(**kw)
    assert net.precision is None and GeneralMLP(**kw, precision="bf16").precision == "bf16"
    assert set(GeneralMLP(**kw, precision="bf16").state_dict()) == set(net.state_dict())     # not part of the state dict
    with pytest.raises(ValueError, match="unknown MLP precision"):
        GeneralMLP(**kw, precision="half")
    net.precision = "bf16"                                                      # may be set later; there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(5, 3))
    w, b = [torch.zeros(64, 20), torch.zeros(64, 64), torch.zeros(3, 64)], [torch.zeros(64), torch.zeros(64), torch.zeros(3)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.fused_general_mlp(torch.zeros(5, 20), w, b, precision="bf16")
    with pytest.raises(ValueError, match="unknown MLP precision"):
        fm.fused_general_mlp(torch.zeros(5, 20), w, b, precision="bfloat16")
    assert fm.FusedGeneralMLP(w, b, 20, precision="bf16").precision == "bf16" and fm.FusedGeneralMLP(w, b, 20).precision is None


def test_environment_variable_sets_the_initial_default(monkeypatch):
    """SPLATFIELDS_MLP_PRECISION is read once, when the module is first imported: a second copy of the module is imported here
    under another name, the package's own copy is not touched"""
    path = os.path.join(ROOT, "splatfields_amd", "fused_mlp.py")

    def fresh(value):
        if value is None:
            monkeypatch.delenv("SPLATFIELDS_MLP_PRECISION", raising=False)
        else:
            monkeypatch.setenv("SPLATFIELDS_MLP_PRECISION", value)
        spec = importlib.util.spec_from_file_location("splatfields_amd._fused_mlp_env_probe", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    assert fresh(None).mlp_precision() == "fp32" and fresh("").mlp_precision() == "fp32"
    assert fresh("fp32").mlp_precision() == "fp32" and fresh("bf16").mlp_precision() == "bf16"
    with pytest.raises(ValueError, match="unknown MLP precision"):
        fresh("fp8")


def test_splatfields_hands_the_precision_to_every_network():
    from splatfields_amd.deform_field import SplatFields
    from splatfields_amd.general_mlp import GeneralMLP
    small = dict(deform_w=64, deform_d=2, deform_skips=[1], rgb_w=64, rgb_d=2, rgb_skips=[0], flow_w=64, flow_d=2, flow_skips=[1],
                 scale_d=2, scale_skips=[0], opacity_d=2, opacity_skips=[5], rotation_d=2, encoder_type="none")
    for precision in (None, "fp32", "bf16"):
        net = SplatFields(n_frames=4, mlp_precision=precision, composition_rank=1, **small)
        inner = [m for m in net.modules() if isinstance(m, GeneralMLP)]
        assert len(inner) == 6 and all(m.precision == precision for m in inner)
    with pytest.raises(ValueError, match="unknown MLP precision"):
        SplatFields(n_frames=0, mlp_precision="fp16", **small)


def test_a_bf16_plan_is_sized_in_bf16_and_stays_16_byte_aligned():
    from splatfields_amd import fused_mlp as fm
    w = [torch.zeros(128, 94), torch.zeros(128, 128), torch.zeros(128, 222), torch.zeros(3, 128)]
    shape = fm._Shape(w, 94, [1])
    sizes = {}
    for precision in fm.PRECISIONS:
        for plan in (fm._forward_plan(shape, True, precision), fm._backward_plan(shape, True, True, precision)):
            assert plan.bf16 == (precision == "bf16")
            plan._freeze()
            jobs, ops, binds, total = plan._arrays
            esize = 2 if plan.bf16 else 4
            at = 0
            base = 1 << 20                                 # patch the buffer's pointers as _Plan.run does, read them back
            for obj, field, sym, idx, off in binds:
                if sym == "buf":
                    setattr(obj, field, base + off)
            for J, O, (wf, bf) in zip(jobs, ops, plan.sizes):
                assert J.dst - base == O.w_packed - base == at and at % 16 == 0
                at += esize * wf
                if bf:
                    assert J.bias_dst - base == O.bias - base == at and at % 16 == 0
                    at += 4 * bf
                else:
                    assert J.bias_dst is None and O.bias is None
            assert total == at and total % 4 == 0
            sizes.setdefault(precision, []).append((total, sum(wf for wf, _ in plan.sizes), sum(bf for _, bf in plan.sizes)))
    for (t32, wf, bf), (t16, wf2, bf2) in zip(sizes["fp32"], sizes["bf16"]):
        assert (wf, bf) == (wf2, bf2) and t32 == 4 * wf + 4 * bf and t16 == 2 * wf + 4 * bf
    assert set(k[-1] for k in shape.plans if k[0] in ("fwd", "bwd")) == {"fp32", "bf16"}      # plans are keyed by precision


def test_bf16_packing_statement_is_the_documented_index_formula():
    """pack_layer_weight_bf16 (the PyTorch statement the device packer is tested against) element by element against the layout
    csrc/mlp.hip documents: bf16 (((c MT + mt) 64 + 16 k + m) 8 + j) = bf(W'[16 mt + m][32 c + 16 (j >> 2) + 4 k + (j & 3)])."""
    from splatfields_amd.fused_mlp import pack_layer_weight_bf16
    g = torch.Generator().manual_seed(2)
    M, n_mem, n_reg, mem_pad, reg_width, MT = 40, 21, 50, 32, 64, 3
    W = torch.randn(M, n_mem + n_reg, generator=g)
    packed = pack_layer_weight_bf16(W, n_mem, mem_pad, reg_width, MT)
    assert packed.dtype == torch.bfloat16 and packed.numel() == 16 * MT * (mem_pad + reg_width)
    Wp = torch.zeros(16 * MT, mem_pad + reg_width)
    Wp[:M, :n_mem] = W[:, :n_mem]
    Wp[:M, mem_pad:mem_pad + n_reg] = W[:, n_mem:]
    Wp = Wp.to(torch.bfloat16)
    for c in range((mem_pad + reg_width) // 32):
        for mt in range(MT):
            for lane in range(64):
                k, m = lane >> 4, lane & 15
                for j in range(8):
                    assert packed[((c * MT + mt) * 64 + lane) * 8 + j] == Wp[16 * mt + m][32 * c + 16 * (j >> 2) + 4 * k + (j & 3)]
