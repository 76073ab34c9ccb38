"""The opt-in split-bf16 ("bf16x3") precision of the fused MLP chains without a GPU: the three C entry points (include/splatraster.h:
sr_mlp_pack_bf16x3 / sr_mlp_chain_bf16x3 / sr_mlp_chain_group_bf16x3) are declared, exported and bound with their bf16 siblings'
signatures, refuse what those refuse with the same words, and leave the ABI version alone; the Python switches accept the name and
hand it to every network; a bf16x3 plan is sized at 4 bytes per weight; the packing statement is the documented index formula.
The kernels themselves: tests/test_gpu_mlp_bf16x3.py."""
import ctypes as C
import importlib.util
import os

import pytest
import torch

import abi_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sr_mlp_pack_bf16x3": "sr_mlp_pack_bf16", "sr_mlp_chain_bf16x3": "sr_mlp_chain_bf16", "sr_mlp_chain_group_bf16x3": "sr_mlp_chain_group_bf16"}


@pytest.fixture(scope="module")
def lib():
    from splatfields_amd import build, _lib
    build.build_library()
    return _lib.load()


def test_symbols_are_declared_exported_bound_and_additions_only(lib):
    from splatfields_amd import _lib
    protos = abi_text.prototypes()
    for new, old in NEW.items():
        assert hasattr(lib, new) and _lib.SYMBOLS[new] == _lib.SYMBOLS[old]        # exported (ctypes resolved it) and bound alike
        assert protos[new] == protos[old]
        text = abi_text.entry_point(new)                                          # defined once, beside its siblings
        assert abi_text.source("mlp.hip").count(text) == 1 and '"%s"' % new in text
    assert protos["sr_mlp_pack_bf16x3"] == ("int", ["int n_jobs", "const SrMlpPackJob* jobs", "void* hip_stream"])
    assert lib.sr_version() == 4 and _lib.SR_VERSION == 4 and abi_text.defines()["SR_VERSION"] == "4"
    # no struct changed: the header's structs are what the binding lays out (field names in order)
    for name in ("SrMlpOp", "SrMlpPackJob", "SrMlpNet"):
        assert [f[1] for f in abi_text.structs()[name]] == [f[0] for f in getattr(_lib, name)._fields_]
    # the siblings' validation is the new entries' validation: one function each, the mode is an argument
    code = abi_text.source("mlp.hip")
    for entry in ("mlp_chain_entry(", "mlp_pack_entry(", "mlp_chain_group_entry("):
        assert code.count(entry) == 4, entry                                       # the definition and one call per precision
    assert code.count("launch_mlp_chain_group(") == 2                              # the definition and mlp_chain_group_entry's call
    assert code.count("static bool mlp_op_ok(") == 1


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


def test_bad_arguments_are_refused_as_by_the_bf16_entry_points(lib):
    """every check precedes the launch: host memory stands in for device memory and is never dereferenced, and there is no device"""
    from splatfields_amd import _lib
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15

    def both(old, new, *args):
        r_old = getattr(lib, old)(*args); e_old = lib.sr_last_error()
        r_new = getattr(lib, new)(*args); e_new = lib.sr_last_error()
        assert r_old != 0 and r_new != 0, args
        assert new.encode() in e_new and e_new.replace(new.encode(), old.encode()) == e_old
        return e_new

    def chain(n_points, ht, ops, slope=0.01, null=False):
        table = (_lib.SrMlpOp * max(len(ops), 1))(*ops)
        return both("sr_mlp_chain_bf16", "sr_mlp_chain_bf16x3", n_points, ht, len(ops), None if null else table, slope, None)

    assert b"bad arguments" in chain(-1, 4, [good_op(p)])
    assert b"bad arguments" in chain(10, 4, [good_op(p)], null=True)
    assert b"negative_slope" in chain(10, 4, [good_op(p)], slope=1.0)
    assert b"negative_slope" in chain(10, 4, [good_op(p)], slope=float("nan"))
    bad_ops = ((5, [good_op(p)]), (4, []), (4, [good_op(p)] * (_lib.MLP_MAX_OPS + 1)), (4, [good_op(p, out_tiles=5)]),
               (4, [good_op(p, mem_tiles=1)]), (4, [good_op(p, mem_tiles=0)]), (4, [good_op(p, reg_tiles=6)]),
               (4, [good_op(p, w_packed=None)]), (4, [good_op(p, w_packed=p + 4)]), (4, [good_op(p, bias=p + 4)]),
               (4, [good_op(p, src=None)]), (4, [good_op(p, src_row=16)]), (4, [good_op(p, epilogue=7)]),
               (4, [good_op(p, epilogue=_lib.MLP_MASK)]), (4, [good_op(p, store_channels=65)]),
               (8, [good_op(p), good_op(p, store_channels=0)]))
    for ht, ops in bad_ops:
        assert b"unsupported op list" in chain(10, ht, ops)

    def pack(jobs, n=None, null=False):
        table = (_lib.SrMlpPackJob * max(len(jobs), 1))(*jobs)
        return both("sr_mlp_pack_bf16", "sr_mlp_pack_bf16x3", len(jobs) if n is None else n, None if null else table, None)

    assert b"bad arguments" in pack([], n=-1)
    assert b"bad arguments" in pack([good_job(p)], null=True)
    for jobs in ([good_job(p)] * (_lib.MLP_MAX_PACK_JOBS + 1), [good_job(p, w=None)], [good_job(p, dst=None)], [good_job(p, dst=p + 8)],
                 [good_job(p, mem_pad=16)], [good_job(p, mem_pad=48)], [good_job(p, reg_width=24)], [good_job(p, n_mem=33)],
                 [good_job(p, n_rows=65)], [good_job(p, out_tiles=0)], [good_job(p, bias_src=None)], [good_job(p, n_bias=65)],
                 [good_job(p), good_job(p, mem_pad=0)]):
        assert b"unsupported job" in pack(jobs)

    def group(n_points, ht, nets_ops, slope=0.01, n_nets=None, null=False):
        tables = [(_lib.SrMlpOp * max(len(ops), 1))(*ops) for ops in nets_ops]
        nets = (_lib.SrMlpNet * max(len(tables), 1))()
        for y, (t, ops) in enumerate(zip(tables, nets_ops)):
            nets[y].ops, nets[y].n_ops = C.cast(t, C.POINTER(_lib.SrMlpOp)), len(ops)
        return both("sr_mlp_chain_group_bf16", "sr_mlp_chain_group_bf16x3", n_points, ht, len(nets_ops) if n_nets is None else n_nets,
                    None if null else nets, slope, None)

    assert b"n_points" in group(-1, 4, [[good_op(p)]])
    assert b"hidden_tiles" in group(10, 5, [[good_op(p)]])
    assert b"negative_slope" in group(10, 4, [[good_op(p)]], slope=1.0)
    assert b"null net table" in group(10, 4, [[good_op(p)]], null=True)
    assert b"SR_MLP_GROUP_MAX_NETS" in group(10, 4, [[good_op(p)]] * (_lib.MLP_GROUP_MAX_NETS + 1))
    assert b"at least one op" in group(10, 4, [[good_op(p)], []])
    assert b"SR_MLP_GROUP_MAX_OPS" in group(10, 4, [[good_op(p)] * 20, [good_op(p)] * 21])
    for ht, ops in bad_ops:
        if ht in (4, 8) and 0 < len(ops) <= _lib.MLP_MAX_OPS:
            assert b"unsupported op" in group(10, ht, [[good_op(p, out_tiles=ht, store_channels=16 * ht, store_row=16 * ht)], ops])
    # valid and empty: success without a device
    one = (_lib.SrMlpNet * 1)()
    assert lib.sr_mlp_chain_group_bf16x3(0, 4, 0, one, 0.01, None) == 0 and lib.sr_mlp_chain_group_bf16x3(10, 8, 0, None, 0.01, None) == 0


def test_the_name_is_accepted_wherever_a_precision_name_is():
    import splatfields_amd
    from splatfields_amd import fused_mlp as fm
    from splatfields_amd.general_mlp import GeneralMLP
    assert fm.PRECISIONS == ("fp32", "bf16") and fm.SPLIT_PRECISIONS == ("bf16x3",)      # the first tuple is walked by older tests
    start = splatfields_amd.mlp_precision()
    try:
        assert splatfields_amd.set_mlp_precision("bf16x3") == start and splatfields_amd.mlp_precision() == "bf16x3"
        assert fm.resolve_precision(None) == "bf16x3" and fm.resolve_precision("bf16") == "bf16"
        with pytest.raises(ValueError, match="unknown MLP precision"):
            splatfields_amd.set_mlp_precision("bf16x2")
        assert splatfields_amd.mlp_precision() == "bf16x3"                     # a refused name changes nothing
        assert splatfields_amd.set_mlp_precision("fp32") == "bf16x3"
    finally:
        splatfields_amd.set_mlp_precision(start)
    kw = dict(in_features=3, out_features=3, hidden_features=64, num_hidden_layers=2, skips=[], multires=2, act="leaky_relu",
              composition_rank=0, n_frames=0)
    net = GeneralMLP(**kw, precision="bf16x3")
    assert net.precision == "bf16x3" and set(net.state_dict()) == set(GeneralMLP(**kw).state_dict())
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.zeros(5, 3))
    w, b = [torch.zeros(64, 20), torch.zeros(64, 64), torch.zeros(3, 64)], [torch.zeros(64), torch.zeros(64), torch.zeros(3)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.fused_general_mlp(torch.zeros(5, 20), w, b, precision="bf16x3")
    with pytest.raises(RuntimeError, match="no CPU path"):
        fm.fused_general_mlp_points(torch.zeros(5, 3), torch.zeros(5, 5), 2, w, b, precision="bf16x3")
    for bad in ("bf16x4", "BF16X3", "split"):
        with pytest.raises(ValueError, match="unknown MLP precision"):
            fm.fused_general_mlp(torch.zeros(5, 20), w, b, precision=bad)
    assert fm.FusedGeneralMLP(w, b, 20, precision="bf16x3").precision == "bf16x3"


def test_environment_variable_sets_the_initial_default(monkeypatch):
    """a second copy of the module is imported under another name; the package's own copy is not touched"""
    monkeypatch.setenv("SPLATFIELDS_MLP_PRECISION", "bf16x3")
    spec = importlib.util.spec_from_file_location("splatfields_amd._fused_mlp_env_probe3", os.path.join(ROOT, "splatfields_amd", "fused_mlp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.mlp_precision() == "bf16x3" and mod.resolve_precision(None) == "bf16x3"
    monkeypatch.setenv("SPLATFIELDS_MLP_PRECISION", "bf16x5")
    with pytest.raises(ValueError, match="unknown MLP precision"):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_splatfields_hands_the_precision_to_every_network():
    from splatfields_amd.deform_field import SplatFields
    from splatfields_amd.general_mlp import GeneralMLP
    small = dict(deform_w=64, deform_d=2, deform_skips=[1], rgb_w=64, rgb_d=2, rgb_skips=[0], flow_w=64, flow_d=2, flow_skips=[1],
                 scale_d=2, scale_skips=[0], opacity_d=2, opacity_skips=[5], rotation_d=2, encoder_type="none")
    for heads in ("separate", "grouped"):
        net = SplatFields(n_frames=4, mlp_precision="bf16x3", composition_rank=1, heads=heads, **small)
        inner = [m for m in net.modules() if isinstance(m, GeneralMLP)]
        assert len(inner) == 6 and all(m.precision == "bf16x3" for m in inner)
    # grouped heads: bf16x3 nets form groups of their own, by (hidden width, precision)
    from splatfields_amd import fused_mlp as fm
    group = net._head_group
    names = [n for g in group.partition() for n in g]
    assert sorted(names) == sorted(group.names) and all(p == "bf16x3" for p in group.spec(tuple("bf16x3" for _ in group.mlps)).precisions)
    mixed = tuple("bf16x3" if i % 2 else "bf16" for i in range(len(group.mlps)))
    for part in group.spec(mixed).groups:
        assert len({mixed[i] for i in part}) == 1
    plans = [fm._forward_plan(group.specs[i].shape, True, "bf16x3") for i in group.spec(tuple("bf16x3" for _ in group.mlps)).groups[0]]
    gp = fm._GroupPlan(plans)
    assert gp.mode == "bf16x3" and gp.bf16 is False
    with pytest.raises(ValueError, match="share one chain precision"):
        fm._GroupPlan([plans[0], fm._forward_plan(group.specs[0].shape, True, "bf16")])


class _Recorder:
    """stands in for the library: records which entry points a plan calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("sr_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append(name) or 0


def test_plans_call_the_entry_points_of_their_precision():
    from splatfields_amd import fused_mlp as fm
    for mode, suffix in (("fp32", ""), ("bf16", "_bf16"), ("bf16x3", "_bf16x3")):
        rec = _Recorder()
        assert tuple(f(0) or rec.calls[-1] for f in fm._entries(rec, mode, group=False)) == ("sr_mlp_pack" + suffix, "sr_mlp_chain" + suffix)
        assert tuple(f(0) or rec.calls[-1] for f in fm._entries(rec, mode, group=True)) == ("sr_mlp_pack" + suffix, "sr_mlp_chain_group" + suffix)
    with pytest.raises(KeyError):
        fm._entries(_Recorder(), "fp16", group=False)


def test_a_bf16x3_plan_is_sized_at_four_bytes_per_weight_and_stays_16_byte_aligned():
    from splatfields_amd import fused_mlp as fm
    w = [torch.zeros(128, 94), torch.zeros(128, 128), torch.zeros(128, 222), torch.zeros(3, 128)]
    shape = fm._Shape(w, 94, [1])
    for make in (lambda p: fm._forward_plan(shape, True, p), lambda p: fm._backward_plan(shape, True, True, p)):
        plan, plain, half = make("bf16x3"), make("fp32"), make("bf16")
        assert plan.mode == "bf16x3" and plan.bf16 is False and plan.wsize == 4 and half.bf16 is True and half.mode == "bf16" and plain.mode == "fp32"
        assert plan is not plain and plan is not half and plan.sizes == plain.sizes
        plan._freeze()
        jobs, ops, binds, total = plan._arrays
        at, base = 0, 1 << 20
        for obj, field, sym, idx, off in binds:
            if sym == "buf":
                setattr(obj, field, base + off)
        for J, O, (wf, bf) in zip(jobs, ops, plan.sizes):
            assert J.dst - base == O.w_packed - base == at and at % 16 == 0
            at += 4 * wf                                   # two bfloat16 per weight
            if bf:
                assert J.bias_dst - base == O.bias - base == at and at % 16 == 0
                at += 4 * bf
            else:
                assert J.bias_dst is None and O.bias is None
        assert total == at and total % 4 == 0
    assert {"fp32", "bf16", "bf16x3"} <= set(k[-1] for k in shape.plans if k[0] in ("fwd", "bwd"))      # plans are keyed by precision


def test_bf16x3_packing_statement_is_the_documented_index_formula():
    """pack_layer_weight_bf16x3 element by element against the layout csrc/mlp_bf16x3.h documents:
    bf16 ((((2 c + part) MT + mt) 64 + 16 k + m) 8 + j) = part(W'[16 mt + m][32 c + 16 (j >> 2) + 4 k + (j & 3)]), hi then lo"""
    from splatfields_amd.fused_mlp import pack_layer_weight_bf16, pack_layer_weight_bf16x3
    g = torch.Generator().manual_seed(2)
    M, n_mem, n_reg, mem_pad, reg_width, MT = 40, 21, 50, 32, 64, 3
    W = torch.randn(M, n_mem + n_reg, generator=g)
    packed = pack_layer_weight_bf16x3(W, n_mem, mem_pad, reg_width, MT)
    assert packed.dtype == torch.bfloat16 and packed.numel() == 2 * 16 * MT * (mem_pad + reg_width)
    Wp = torch.zeros(16 * MT, mem_pad + reg_width)
    Wp[:M, :n_mem] = W[:, :n_mem]
    Wp[:M, mem_pad:mem_pad + n_reg] = W[:, n_mem:]
    hi = Wp.to(torch.bfloat16)
    lo = (Wp - hi.float()).to(torch.bfloat16)
    assert (lo != 0).float().mean() > 0.5 and ((hi.float() + lo.float() - Wp).abs() <= 2.0 ** -16 * Wp.abs()).all()
    flat = packed.tolist()
    parts = (hi.tolist(), lo.tolist())
    for c in range((mem_pad + reg_width) // 32):
        for part in range(2):
            for mt in range(MT):
                for lane in range(64):
                    k, m = lane >> 4, lane & 15
                    for j in range(8):
                        assert flat[(((2 * c + part) * MT + mt) * 64 + lane) * 8 + j] == parts[part][16 * mt + m][32 * c + 16 * (j >> 2) + 4 * k + (j & 3)]
    # the hi blocks are the bf16 packing, chunk by chunk
    plain = pack_layer_weight_bf16(W, n_mem, mem_pad, reg_width, MT).view(-1, MT * 512)
    assert torch.equal(packed.view(-1, 2, MT * 512)[:, 0].contiguous().view(torch.int16), plain.view(torch.int16))
