"""CPU: the C-ABI library loads and exports every symbol include/vilco_hip.h declares; argument
validation paths that need no GPU; the config surface equals the reference DEFAULTS."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "vilco_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vilco_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    from vilco_amd import _lib
    names = declared_symbols()
    assert len(names) >= 25
    assert sorted(_lib.SIGNATURES) == names, "ctypes table and header disagree"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "missing export " + n


def test_status_strings_and_version():
    from vilco_amd import _lib
    lib = _lib.load()
    assert b"gfx950" in lib.vilco_version()
    assert lib.vilco_status_str(0) == b"ok"
    for code in (-1, -2, -3, -4):
        assert lib.vilco_status_str(code).startswith(b"vilco_hip")


def test_bad_arguments_are_rejected_without_a_gpu():
    from vilco_amd import _lib
    lib = _lib.load()
    d = _lib.GemmDesc()
    assert lib.vilco_gemm(ctypes.byref(d), None) == -1              # null operands
    assert lib.vilco_layernorm_fwd(ctypes.byref(_lib.LnFwdDesc(rows=4, C=64, eps=1e-5)), None) == -1     # null operands
    assert lib.vilco_layernorm_fwd(None, None) == -1
    assert lib.vilco_nms_1d(None, None, None, -1, 0, 0.5, None, None, None, 0, None) == -1
    with pytest.raises(RuntimeError, match="bad argument"):
        _lib.check(-1)
    # an operand matrix of 2^31 bytes or more is refused (the kernel's staging loads carry 32-bit byte offsets); the check
    # comes before anything touches memory, so dummy addresses do
    d = _lib.GemmDesc()
    d.A = d.B = d.C = 4096
    d.M, d.N, d.K = 70000, 128, 20000
    d.a_kcontig = d.b_kcontig = 1
    d.lda = d.ldb = 20000
    d.ldc = 128
    d.batch_outer = d.batch_inner = 1
    d.precision = 3
    assert lib.vilco_gemm(ctypes.byref(d), None) == -2
    d.M = 7000                                                  # the same call with a legal size gets as far as the workspace check
    assert lib.vilco_gemm(ctypes.byref(d), None) == -4


def test_ops_refuse_cpu_tensors():
    import torch
    from vilco_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear(torch.zeros(4, 8), torch.zeros(3, 8))


def test_config_defaults_match_reference():
    import torch
    from vilco_amd.core import config as c
    cfg = c.make_config(dataset=dict(input_dim=96))
    assert cfg["model"]["input_dim"] == 96 and cfg["model"]["train_cfg"] is cfg["train_cfg"]
    # the reference's DEFAULTS, recorded by tests/golden/make_golden_defaults.py
    ref_defaults = torch.load(os.path.join(ROOT, "tests", "golden", "config_defaults.pt"), weights_only=False)
    assert c.DEFAULTS == ref_defaults


def test_state_dict_is_drop_in():
    """same keys and shapes as the golden reference state_dict; loads strictly"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from parity_util import golden_cfg, load_golden, xlnet_json
    import vilco_amd.modeling as vm
    for name in ("xl", "prompt"):
        gold = load_golden(name)
        m = golden_cfg(gold)
        kw = dict(m, xlnet_config=xlnet_json(m['embd_dim'], 4)) if m['use_xl'] else m
        model = vm.make_meta_arch('LocPointTransformer', **kw)
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == \
               {k: tuple(v.shape) for k, v in gold['state_dict'].items()}
        model.load_state_dict(gold['state_dict'], strict=True)


def test_producer_plane_entry_points_validate_on_the_host():
    """the producer-written-planes entry points (round 4): buffer sizes equal the pack's for the same tensor, and bad layouts are
    refused before anything is launched"""
    from vilco_amd import _lib
    lib = _lib.load()
    for rows, C in ((4608, 1024), (100, 96), (77, 32)):
        assert lib.vilco_layernorm_planes_bytes(rows, C, 0) == lib.vilco_pack_bytes(rows, C, 3)
    it = _lib.PackItem()
    it.rows, it.cols, it.ld, it.nbatch, it.seq_len = 2 * 4541, 1024, 1024, 1, 4541
    assert lib.vilco_layernorm_planes_bytes(2 * 4541, 1024, 4541) == lib.vilco_pack_item_bytes(ctypes.byref(it), 3)
    x = 4096                                            # dummy, suitably aligned addresses: every check below precedes the launch
    # natural planes need C % 32 == 0, the convs' image whole sequences; a short buffer is a workspace error
    def ln_fwd(**kw):
        d = _lib.LnFwdDesc(x=x, y=x, mean=x, rstd=x, eps=1e-5, planes=x, **kw)
        return lib.vilco_layernorm_fwd(ctypes.byref(d), None)
    assert ln_fwd(rows=64, C=40, planes_bytes=1 << 30) == -2
    assert ln_fwd(rows=65, C=64, planes_bytes=1 << 30, seq_len=16) == -2
    assert ln_fwd(rows=64, C=64, planes_bytes=128) == -4
    # activation backward: planes need the partial maxima of dy, C % 32 == 0 and a buffer of vilco_pack_bytes

    def act_bwd(**kw):
        d = _lib.ActBwdDesc(dy=x, rows=64, planes=x, **kw)
        return lib.vilco_act_bwd(ctypes.byref(d), None)
    assert act_bwd(C=64, planes_bytes=1 << 30) == -1
    assert act_bwd(C=40, planes_bytes=1 << 30, dy_amax=x, n_dy_amax=4) == -1
    assert act_bwd(C=64, planes_bytes=128, dy_amax=x, n_dy_amax=4) == -4
    # a row mask on a batched product is not supported
    d = _lib.GemmDesc()
    d.A = d.B = d.C = d.row_mask = 4096
    d.M, d.N, d.K = 128, 128, 64
    d.a_kcontig = d.b_kcontig = 1
    d.lda = d.ldb = 64
    d.ldc = 128
    d.batch_outer, d.batch_inner, d.precision = 2, 1, 3
    assert lib.vilco_gemm(ctypes.byref(d), None) == -2


def test_optional_parts_of_the_descriptors_validate_on_the_host():
    """what the descriptors' optional fields exclude, refused before anything is launched (dummy aligned addresses)"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096
    # XLNet's relative attention at hd = 64 (mask mode 3, bias, precision 3): dS leaves either as dbias or as ds_planes, not both
    xl = dict(q=x, k=x, v=x, bias=x, kv_len=x, o=x, lse=x, B=1, H=1, Tq=64, Tk=64, scale=0.125, mode=3, precision=3,
              workspace=x, workspace_bytes=1 << 40)
    d = _lib.AttnDesc(hd=64, dout=x, dq=x, dk=x, dv=x, dbias=x, ds_planes=x, ds_planes_bytes=1 << 40, **xl)
    assert lib.vilco_attn_bwd(ctypes.byref(d), None) == -2
    # the output's operand planes come from the hd = 64 forward kernels only
    d = _lib.AttnDesc(hd=32, o_planes=x, o_planes_bytes=1 << 40, **xl)
    assert lib.vilco_attn_fwd(ctypes.byref(d), None) == -2
    # at most 8 parameter groups travel as kernel arguments
    lr = (ctypes.c_float * 9)()
    tb = _lib.ChunkTable(ptrs=x, numel=x, chunk_tensor=x, chunk_off=x, rows=4, n=1, nchunks=1, chunk=1024)
    d = _lib.OptimDesc(table=tb, group=x, lr=ctypes.addressof(lr), wd=ctypes.addressof(lr), ngroups=9, tensor_step=x)
    assert lib.vilco_optim_step(ctypes.byref(d), None) == -1
    # LayerNorm backward: dgamma and dbeta come together or not at all
    d = _lib.LnBwdDesc(dy=x, x=x, mean=x, rstd=x, dx=x, dgamma=x, rows=64, C=64, workspace=x, workspace_bytes=1 << 40)
    assert lib.vilco_layernorm_bwd(ctypes.byref(d), None) == -1


def test_struct_mirrors_have_the_size_the_compiler_gave_the_c_structs():
    from vilco_amd import _lib
    lib = _lib.load()
    mirrors = [c for c in vars(_lib).values() if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure]
    assert len(mirrors) >= 10
    for c in mirrors:
        assert ctypes.sizeof(c) == lib.vilco_abi_sizeof(c._cname_.encode()) > 0, c.__name__
    assert lib.vilco_abi_sizeof(b"vilco_no_such_struct") == 0


def test_chunk_table_entry_points_validate_on_the_host():
    """vilco_grad_norm and vilco_cl_penalty (the other three users of a vilco_chunk_table: test_importance_cpu.py,
    test_si_cpu.py): a null table, null rows of it, bad counts and one row too few are refused before anything is launched"""
    from vilco_amd import _lib
    lib = _lib.load()
    x = 4096
    ok = dict(ptrs=x, numel=x, chunk_tensor=x, chunk_off=x, n=1, nchunks=1, chunk=1024)
    calls = {"grad_norm": (2, lambda t: lib.vilco_grad_norm(t, 0.5, x, x, None)),
             "cl_penalty": (4, lambda t: lib.vilco_cl_penalty(t, 0.37, 0, x, x, None))}
    for name, (rows, call) in calls.items():
        assert call(None) == -1, name
        for bad in (dict(ptrs=None), dict(numel=None), dict(chunk_tensor=None), dict(chunk_off=None), dict(n=-1), dict(nchunks=-1),
                    dict(chunk=0), dict(rows=rows - 1)):
            assert call(ctypes.byref(_lib.ChunkTable(**dict(dict(ok, rows=rows), **bad)))) == -1, (name, bad)
    tb = ctypes.byref(_lib.ChunkTable(rows=4, **ok))
    assert lib.vilco_grad_norm(tb, 0.5, None, x, None) == -1 and lib.vilco_grad_norm(tb, 0.5, x, None, None) == -1
    assert lib.vilco_cl_penalty(tb, 0.37, 0, None, x, None) == -1 and lib.vilco_cl_penalty(tb, 0.37, 0, x, None, None) == -1
    assert ctypes.sizeof(_lib.ChunkTable) == lib.vilco_abi_sizeof(b"vilco_chunk_table") == 48
    assert _lib.OptimDesc._fields_[0] == ("table", _lib.ChunkTable) and _lib.SiDesc._fields_[0] == ("table", _lib.ChunkTable)


def test_chunk_plan_is_the_table_the_tests_build_by_hand():
    """ops.ChunkPlan against tests/optim_restatement.py's own loop, at the chunk edges and for no tensors at all"""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import optim_restatement as R
    from vilco_amd import ops
    from vilco_amd.cl_methods import regularizers
    from vilco_amd.utils import train_utils
    assert ops.CHUNK == R.CHUNK and ops.CL_CHUNK is ops.CHUNK and train_utils.CHUNK is ops.CHUNK and regularizers.CHUNK is ops.CHUNK
    C = R.CHUNK
    for numels in ([], [1, 3, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5]):
        ct, co, first = R.chunk_lists(numels)
        plan = ops.ChunkPlan(numels, torch.device('cpu'))
        assert (plan.n, plan.nchunks, plan.chunk, plan.first) == (len(numels), len(ct), C, first)
        assert plan.numel.dtype == torch.int64 and plan.chunk_tensor.dtype == torch.int32 and plan.chunk_off.dtype == torch.int64
        assert plan.numel.tolist() == (numels or [0]) and plan.chunk_tensor.tolist() == (ct or [0]) and plan.chunk_off.tolist() == (co or [0])
        ptrs = torch.zeros(3, max(len(numels), 1), dtype=torch.int64)
        t = plan.table(ptrs, 3)
        assert (t.ptrs, t.numel, t.chunk_tensor, t.chunk_off) == (ptrs.data_ptr(), plan.numel.data_ptr(), plan.chunk_tensor.data_ptr(),
                                                                   plan.chunk_off.data_ptr())
        assert (t.rows, t.n, t.nchunks, t.chunk) == (3, len(numels), len(ct), C) and t.chunk_off
    assert first == [0, 1, 2, 3, 4, 5, 6, 7, 9, 12] and co[-3:] == [0, C, 2 * C] and ct[-3:] == [8, 8, 8]
