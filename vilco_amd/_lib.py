"""ctypes binding of libvilco_hip.so (C ABI: include/vilco_hip.h).

The product path has NO fallback: if the library is missing or a kernel returns a status, we
raise.  `load()` is lazy so that CPU-only tooling (config parsing, state_dict surgery, the
`-m "not gpu"` symbol test) can import the package without a GPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
if __package__:
    from . import switches
else:       # loaded alone by file path (ctypes-only child processes that must not import the package, which imports torch)
    import importlib.util
    _spec = importlib.util.spec_from_file_location("vilco_switches", os.path.join(_HERE, "switches.py"))
    switches = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(switches)
LIB_PATH = switches.text("VILCO_HIP_LIB") or os.path.join(_HERE, "libvilco_hip.so")   # override: tools/lab builds

ACT_NONE, ACT_RELU, ACT_GELU = 0, 1, 2
TAP_NONE, TAP_A, TAP_B = 0, 1, 2

c_fp = C.c_void_p   # device pointers travel as integers (tensor.data_ptr())
i32, i64, f32, sz = C.c_int32, C.c_int64, C.c_float, C.c_size_t


# Every Structure below mirrors the C struct `_cname_` of include/vilco_hip.h field for field; tests/test_cabi_cpu.py holds
# each to the size the library reports for that name (vilco_abi_sizeof).
class GemmDesc(C.Structure):
    _cname_ = "vilco_gemm_desc"
    _fields_ = [
        ("A", c_fp), ("B", c_fp), ("C", c_fp),
        ("M", i32), ("N", i32), ("K", i32),
        ("a_kcontig", i32), ("b_kcontig", i32),
        ("lda", i64), ("ldb", i64), ("ldc", i64),
        ("batch_outer", i32), ("batch_inner", i32),
        ("sAo", i64), ("sAi", i64), ("sBo", i64), ("sBi", i64), ("sCo", i64), ("sCi", i64),
        ("tap_operand", i32), ("tapC", i32), ("tapT", i32),
        ("precision", i32),
        ("alpha", f32), ("beta", f32),
        ("bias", c_fp), ("preact", c_fp), ("act", i32),
        ("row_len", c_fp), ("rowT", i32),
        ("colscale", c_fp), ("residual", c_fp), ("res_masked", i32),
        ("workspace", c_fp), ("workspace_bytes", sz),
        ("a_planes", c_fp), ("b_planes", c_fp),
        ("band", i32), ("bandT", i32),
        ("drop_p", f32), ("drop_seed", C.c_uint32),
        ("amax_out", c_fp),
        ("a_amax", c_fp), ("a_namax", i32), ("b_amax", c_fp), ("b_namax", i32),
        ("a_planes_seq", i32), ("b_planes_seq", i32),
        ("row_mask", c_fp),
    ]


class LossDesc(C.Structure):
    _cname_ = "vilco_loss_desc"
    _fields_ = [("logits", c_fp), ("offsets", c_fp), ("level_scale", c_fp), ("points", c_fp), ("row_level", c_fp),
                ("row_pos", c_fp), ("level_len", c_fp), ("gt", c_fp), ("gauss", c_fp), ("loss_norm", c_fp),
                ("B", i32), ("R", i32), ("C", i32), ("L", i32), ("Nmax", i32),
                ("center_radius", f32), ("label_smoothing", f32), ("momentum", f32), ("loss_weight", f32),
                ("al_weight", f32), ("use_al", i32)]


class AttnAmaxIn(C.Structure):
    _cname_ = "vilco_attn_amax_in"
    _fields_ = [("q", c_fp), ("nq", i32), ("k", c_fp), ("nk", i32), ("v", c_fp), ("nv", i32), ("dout", c_fp), ("ndo", i32)]


class PackItem(C.Structure):
    _cname_ = "vilco_pack_item"
    _fields_ = [("src", c_fp), ("rows", i64), ("cols", i64), ("ld", i64), ("planes", c_fp), ("planes_bytes", sz),
                ("nbatch", i32), ("batch_stride", i64), ("relshift", i32), ("amax", c_fp), ("namax", i32), ("seq_len", i32)]


# host addresses travel as integers too (C.addressof): the `n_parts` c_int32 a call writes, AttnDesc.amax_in, OptimDesc.lr / wd
class LnFwdDesc(C.Structure):
    _cname_ = "vilco_ln_fwd_desc"
    _fields_ = [("x", c_fp), ("gamma", c_fp), ("beta", c_fp), ("y", c_fp), ("mean", c_fp), ("rstd", c_fp),
                ("rows", i64), ("C", i32), ("eps", f32), ("relu", i32), ("amax_parts", c_fp), ("n_parts", c_fp),
                ("planes", c_fp), ("planes_bytes", sz), ("seq_len", i32), ("row_mask", c_fp), ("mask_rows", i64)]


class LnBwdDesc(C.Structure):
    _cname_ = "vilco_ln_bwd_desc"
    _fields_ = [("dy", c_fp), ("x", c_fp), ("y", c_fp), ("gamma", c_fp), ("mean", c_fp), ("rstd", c_fp), ("dres", c_fp),
                ("dx", c_fp), ("dgamma", c_fp), ("dbeta", c_fp), ("rows", i64), ("C", i32), ("relu", i32),
                ("workspace", c_fp), ("workspace_bytes", sz), ("dx_amax_parts", c_fp), ("n_parts", c_fp)]


class AttnDesc(C.Structure):
    _cname_ = "vilco_attn_desc"
    _fields_ = [("q", c_fp), ("k", c_fp), ("v", c_fp), ("bias", c_fp), ("kv_len", c_fp), ("o", c_fp), ("lse", c_fp),
                ("B", i32), ("H", i32), ("Tq", i32), ("Tk", i32), ("hd", i32), ("scale", f32),
                ("mode", i32), ("window", i32), ("precision", i32), ("drop_p", f32), ("drop_seed", C.c_uint32),
                ("amax_in", c_fp), ("workspace", c_fp), ("workspace_bytes", sz),
                ("o_amax", c_fp), ("o_planes", c_fp), ("o_planes_bytes", sz),
                ("dout", c_fp), ("dq", c_fp), ("dk", c_fp), ("dv", c_fp), ("dbias", c_fp),
                ("dq_amax", c_fp), ("dk_amax", c_fp), ("dv_amax", c_fp), ("dbias_amax", c_fp),
                ("ds_planes", c_fp), ("ds_planes_bytes", sz)]


class ScaleAddBwdDesc(C.Structure):
    _cname_ = "vilco_scale_add_bwd_desc"
    _fields_ = [("dout", c_fp), ("bval", c_fp), ("colscale", c_fp), ("rowscale", c_fp), ("len", c_fp), ("mask_a", i32),
                ("da", c_fp), ("db", c_fp), ("dcolscale", c_fp), ("B", i32), ("T", i32), ("C", i32),
                ("workspace", c_fp), ("workspace_bytes", sz), ("db_amax_parts", c_fp), ("n_parts", c_fp)]


class ActBwdDesc(C.Structure):
    _cname_ = "vilco_act_bwd_desc"
    _fields_ = [("dy", c_fp), ("aux", c_fp), ("dz", c_fp), ("dbias", c_fp), ("act", i32), ("len", c_fp), ("T", i32),
                ("rows", i64), ("C", i32), ("drop_p", f32), ("drop_seed", C.c_uint32),
                ("workspace", c_fp), ("workspace_bytes", sz), ("amax_parts", c_fp), ("n_parts", c_fp),
                ("dy_amax", c_fp), ("n_dy_amax", i32), ("planes", c_fp), ("planes_bytes", sz), ("seq_len", i32),
                ("row_mask", c_fp)]


class ChunkTable(C.Structure):
    _cname_ = "vilco_chunk_table"
    _fields_ = [("ptrs", c_fp), ("numel", c_fp), ("chunk_tensor", c_fp), ("chunk_off", c_fp),
                ("rows", i32), ("n", i32), ("nchunks", i32), ("chunk", i32)]


class OptimDesc(C.Structure):
    _cname_ = "vilco_optim_desc"
    _fields_ = [("table", ChunkTable), ("kind", i32), ("group", c_fp), ("lr", c_fp), ("wd", c_fp), ("ngroups", i32),
                ("beta1", f32), ("beta2", f32), ("eps", f32), ("momentum", f32), ("tensor_step", c_fp), ("norm_coef", c_fp),
                ("chunk_amax", c_fp), ("lr_dev", c_fp), ("si_ptrs", c_fp)]


class SiDesc(C.Structure):
    _cname_ = "vilco_si_desc"
    _fields_ = [("table", ChunkTable), ("numel_old", c_fp), ("xi", f32)]


class RwalkStepDesc(C.Structure):
    _cname_ = "vilco_rwalk_step_desc"
    _fields_ = [("optim", OptimDesc), ("rw_ptrs", c_fp), ("tick", c_fp), ("alpha", f32), ("eps", f32), ("delta_t", i32)]


class RwalkDesc(C.Structure):
    _cname_ = "vilco_rwalk_desc"
    _fields_ = [("table", ChunkTable), ("out_ptrs", c_fp), ("partial", c_fp), ("out", c_fp), ("eps", f32)]


class DistillDesc(C.Structure):
    _cname_ = "vilco_distill_desc"
    _fields_ = [("logits", c_fp), ("targets", c_fp), ("level_row", c_fp), ("level_T", c_fp), ("level_dev", c_fp),
                ("B", i32), ("R", i32), ("C", i32), ("L", i32), ("clip", i32), ("ldt", i32), ("n_known", i32), ("mode", i32),
                ("scale", f32)]


class DerDesc(C.Structure):
    _cname_ = "vilco_der_desc"
    _fields_ = [("logits", c_fp), ("level_row", c_fp), ("level_T", c_fp), ("level_dev", c_fp), ("level_len", c_fp),
                ("der_tab", c_fp), ("B", i32), ("R", i32), ("C", i32), ("L", i32), ("alpha", C.c_double)]


class PodDesc(C.Structure):
    _cname_ = "vilco_pod_desc"
    _fields_ = [("feats", c_fp), ("level_T", c_fp), ("level_len", c_fp), ("pod_tab", c_fp), ("B", i32), ("C", i32), ("L", i32),
                ("reserved", i32), ("scale", C.c_double)]


class ErdDesc(C.Structure):
    _cname_ = "vilco_erd_desc"
    _fields_ = [("logits", c_fp), ("offsets", c_fp), ("scale", c_fp), ("level_row", c_fp), ("level_T", c_fp), ("level_dev", c_fp),
                ("level_len", c_fp), ("erd_tab", c_fp), ("B", i32), ("R", i32), ("C", i32), ("L", i32),
                ("lambda_cls", C.c_double), ("lambda_reg", C.c_double)]


class ErdSelectDesc(C.Structure):
    _cname_ = "vilco_erd_select_desc"
    _fields_ = [("logits", c_fp), ("offsets", c_fp), ("level_T", c_fp), ("level_len", c_fp), ("conf", c_fp), ("flags", c_fp),
                ("counts", c_fp), ("out_tab", c_fp), ("B", i32), ("P", i32), ("C", i32), ("n_old", i32), ("L", i32),
                ("reserved", i32), ("alpha_cls", C.c_double), ("alpha_reg", C.c_double)]


class BicCorrectDesc(C.Structure):
    _cname_ = "vilco_bic_correct_desc"
    _fields_ = [("x", c_fp), ("y", c_fp), ("splits", c_fp), ("table", c_fp), ("rows", i64), ("C", i32), ("S", i32),
                ("ldx", i32), ("ldy", i32), ("n_layers", i32)]


class PromptDesc(C.Structure):
    _cname_ = "vilco_prompt_desc"
    _fields_ = [("x", c_fp), ("prompt", c_fp), ("key", c_fp), ("cls", c_fp), ("idx_in", c_fp),
                ("B", i32), ("L", i32), ("C", i32), ("P", i32), ("len", i32), ("k", i32), ("key_mode", i32), ("vote", i32),
                ("idx", c_fp), ("sim", c_fp), ("pn", c_fp), ("xn", c_fp), ("selkey", c_fp), ("prompted", c_fp),
                ("reduce_sim", c_fp), ("workspace", c_fp), ("workspace_bytes", sz)]


class CodaDesc(C.Structure):
    _cname_ = "vilco_coda_desc"
    _fields_ = [("x", c_fp), ("prompt", c_fp), ("key", c_fp), ("attn", c_fp),
                ("B", i32), ("L", i32), ("C", i32), ("M", i32), ("len", i32), ("s", i32), ("f", i32), ("want_ortho", i32),
                ("alpha", c_fp), ("prompted", c_fp), ("ortho", c_fp), ("workspace", c_fp), ("workspace_bytes", sz)]


# name -> (restype, argtypes); must list every symbol include/vilco_hip.h declares
SIGNATURES = {
    "vilco_status_str": (C.c_char_p, [C.c_int]),
    "vilco_version": (C.c_char_p, []),
    "vilco_abi_sizeof": (sz, [C.c_char_p]),
    "vilco_defer_set": (C.c_int, [i32]),
    "vilco_defer_pending": (i64, []),
    "vilco_defer_flush": (C.c_int, [c_fp]),
    "vilco_gemm_workspace": (sz, [C.POINTER(GemmDesc)]),
    "vilco_gemm": (C.c_int, [C.POINTER(GemmDesc), c_fp]),
    "vilco_gemm_group": (C.c_int, [C.POINTER(GemmDesc), i32, c_fp]),
    "vilco_gemm_group_workspace": (sz, [C.POINTER(GemmDesc), i32]),
    "vilco_gemm_set_group_dw": (C.c_int, [i32]),
    "vilco_gemm_group_dw": (i32, []),
    "vilco_gemm_amax_parts": (i32, [C.POINTER(GemmDesc)]),
    "vilco_gemm_force": (C.c_int, [i32, i32]),
    "vilco_gemm_set_skinny": (C.c_int, [i32]),
    "vilco_gemm_config_gen": (i64, []),
    "vilco_gemm_profile_begin": (C.c_int, []),
    "vilco_gemm_profile_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "vilco_gemm_profile_records": (C.c_int64, [C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int64]),
    "vilco_pack_bytes": (sz, [i64, i64, i32]),
    "vilco_pack_item_bytes": (sz, [C.POINTER(PackItem), i32]),
    "vilco_pack": (C.c_int, [c_fp, i64, i64, i64, i32, c_fp, sz, c_fp]),
    "vilco_pack_many": (C.c_int, [C.POINTER(PackItem), i32, i32, c_fp]),
    "vilco_layernorm_fwd": (C.c_int, [C.POINTER(LnFwdDesc), c_fp]),
    "vilco_layernorm_planes_bytes": (sz, [i64, i32, i32]),
    "vilco_layernorm_bwd_workspace": (sz, [i64, i32]),
    "vilco_layernorm_bwd": (C.c_int, [C.POINTER(LnBwdDesc), c_fp]),
    "vilco_dwconv3_fwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, i32, i32, i32, i32, c_fp]),
    "vilco_dwconv3_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "vilco_dwconv3_bwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, i32, i32, i32, i32, c_fp, sz, c_fp]),
    "vilco_maxpool3s2_fwd": (C.c_int, [c_fp, c_fp, c_fp, i32, i32, i32, c_fp]),
    "vilco_maxpool3s2_bwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, i32, i32, i32, c_fp]),
    "vilco_softmax_fwd": (C.c_int, [c_fp, c_fp, i32, i32, i32, i32, i32, c_fp]),
    "vilco_softmax_bwd": (C.c_int, [c_fp, c_fp, i32, i32, i32, i32, c_fp]),
    "vilco_relshift_add": (C.c_int, [c_fp, c_fp, f32, i32, i32, i32, c_fp]),
    "vilco_relshift_bwd": (C.c_int, [c_fp, c_fp, f32, i32, i32, i32, c_fp]),
    "vilco_attn_supported": (C.c_int, [i32]),
    "vilco_attn_fwd_workspace": (sz, [i32, i32, i32, i32, i32, i32]),
    "vilco_attn_amax_parts": (i32, [i32, i32, i32, i32, i32, i32, i32, f32, i32]),
    "vilco_attn_fwd": (C.c_int, [C.POINTER(AttnDesc), c_fp]),
    "vilco_attn_planes_supported": (i32, [i32, i32, i32, i32, i32, i32, f32]),
    "vilco_attn_bwd_workspace": (sz, [i32, i32, i32, i32, i32, i32]),
    "vilco_attn_bwd": (C.c_int, [C.POINTER(AttnDesc), c_fp]),
    "vilco_attn_dsplanes_bytes": (sz, [i32, i32, i32]),
    "vilco_xl_scores_workspace": (sz, [i32, i32, i32, i32]),
    "vilco_xl_scores": (C.c_int, [c_fp, c_fp, c_fp, i32, i32, i32, i32, i32, i32, c_fp, sz, c_fp]),
    "vilco_decode_workspace": (sz, [i32, i32]),
    "vilco_decode": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, i32, i32, i32, f32, f32, c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_scale_add_fwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, i32, i32, i32, i32, c_fp]),
    "vilco_colsum_workspace": (sz, [i64, i32]),
    "vilco_scale_add_bwd": (C.c_int, [C.POINTER(ScaleAddBwdDesc), c_fp]),
    "vilco_dropout": (C.c_int, [c_fp, c_fp, i64, f32, C.c_uint32, C.c_uint64, c_fp]),
    "vilco_attn_dropout_mask": (C.c_int, [c_fp, i64, i32, f32, C.c_uint32, c_fp]),
    "vilco_seed_word_set": (C.c_int, [C.c_uint32, c_fp]),
    "vilco_seed_word_bump": (C.c_int, [c_fp]),
    "vilco_seed_word_get": (C.c_int, [C.POINTER(C.c_uint32)]),
    "vilco_axpby": (C.c_int, [c_fp, c_fp, c_fp, f32, f32, i64, c_fp]),
    "vilco_act_bwd": (C.c_int, [C.POINTER(ActBwdDesc), c_fp]),
    "vilco_act_bwd_planes_bytes": (sz, [i64, i32, i32]),
    "vilco_colsum": (C.c_int, [c_fp, c_fp, i64, i32, c_fp, sz, c_fp]),
    "vilco_mask_rows": (C.c_int, [c_fp, c_fp, i32, i32, i32, c_fp]),
    "vilco_add_pe": (C.c_int, [c_fp, c_fp, c_fp, c_fp, i32, i32, i32, c_fp]),
    "vilco_transpose2d": (C.c_int, [c_fp, c_fp, i32, i32, i32, c_fp]),
    "vilco_permute3": (C.c_int, [c_fp, c_fp, i32, i32, i32, i64, i64, i64, i64, c_fp]),
    "vilco_grad_norm": (C.c_int, [C.POINTER(ChunkTable), f32, c_fp, c_fp, c_fp]),
    "vilco_optim_step": (C.c_int, [C.POINTER(OptimDesc), c_fp]),
    "vilco_si_consolidate": (C.c_int, [C.POINTER(SiDesc), c_fp]),
    "vilco_optim_step_rwalk": (C.c_int, [C.POINTER(RwalkStepDesc), c_fp]),
    "vilco_rwalk_consolidate": (C.c_int, [C.POINTER(RwalkDesc), c_fp]),
    "vilco_store_f32": (C.c_int, [c_fp, C.POINTER(f32), i32, c_fp]),
    "vilco_qkv_pre_supported": (C.c_int, [i32]),
    "vilco_qkv_pre_amax_parts": (C.c_int, [i32, i32, i32]),
    "vilco_qkv_pre_fwd": (C.c_int, [c_fp, c_fp, c_fp, C.POINTER(c_fp), C.POINTER(c_fp), C.POINTER(c_fp), c_fp, c_fp,
                                    C.POINTER(c_fp), c_fp, c_fp, C.POINTER(c_fp), C.POINTER(c_fp), C.POINTER(c_fp), i32, i32,
                                    i32, i32, f32, f32, c_fp]),
    "vilco_qkv_pre_bwd_workspace": (sz, [i32, i32, i32, i32]),
    "vilco_qkv_pre_bwd": (C.c_int, [c_fp, C.POINTER(c_fp), C.POINTER(c_fp), C.POINTER(c_fp), C.POINTER(c_fp),
                                    C.POINTER(c_fp), c_fp, c_fp, C.POINTER(c_fp), c_fp, c_fp, i32, i32, i32, i32, c_fp, sz,
                                    c_fp]),
    "vilco_mq_loss_workspace": (sz, [i32, i32, i32]),
    "vilco_mq_loss_fwd": (C.c_int, [C.POINTER(LossDesc), c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_mq_loss_bwd": (C.c_int, [C.POINTER(LossDesc), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp,
                                    c_fp]),
    "vilco_mq_loss_ace_fwd": (C.c_int, [C.POINTER(LossDesc), c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_mq_loss_ace_bwd": (C.c_int, [C.POINTER(LossDesc), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp,
                                        c_fp, c_fp]),
    "vilco_cl_distill_workspace": (sz, [i64]),
    "vilco_cl_distill_fwd": (C.c_int, [C.POINTER(DistillDesc), c_fp, c_fp, sz, c_fp]),
    "vilco_cl_distill_bwd": (C.c_int, [C.POINTER(DistillDesc), c_fp, c_fp, c_fp]),
    "vilco_der_workspace": (sz, [i64]),
    "vilco_der_fwd": (C.c_int, [C.POINTER(DerDesc), c_fp, c_fp, sz, c_fp]),
    "vilco_der_bwd": (C.c_int, [C.POINTER(DerDesc), c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_pod_tile_rows": (i32, []),
    "vilco_pod_workspace": (sz, [C.POINTER(i32), i32, i32, i32]),
    "vilco_pod_fwd": (C.c_int, [C.POINTER(PodDesc), c_fp, c_fp, sz, c_fp]),
    "vilco_pod_bwd": (C.c_int, [C.POINTER(PodDesc), c_fp, C.POINTER(c_fp), c_fp, sz, c_fp]),
    "vilco_pod_record": (C.c_int, [C.POINTER(PodDesc), c_fp, c_fp, sz, c_fp]),
    "vilco_erd_pairs_per_round": (i32, []),
    "vilco_erd_workspace": (sz, [i64]),
    "vilco_erd_fwd": (C.c_int, [C.POINTER(ErdDesc), c_fp, c_fp, sz, c_fp]),
    "vilco_erd_bwd": (C.c_int, [C.POINTER(ErdDesc), c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_erd_select": (C.c_int, [C.POINTER(ErdSelectDesc), c_fp]),
    "vilco_erd_select_fill": (C.c_int, [C.POINTER(ErdSelectDesc), c_fp]),
    "vilco_cl_penalty": (C.c_int, [C.POINTER(ChunkTable), f32, i32, c_fp, c_fp, c_fp]),
    "vilco_cl_accumulate": (C.c_int, [C.POINTER(ChunkTable), i32, f32, f32, c_fp]),
    "vilco_agem_project": (C.c_int, [C.POINTER(ChunkTable), c_fp, c_fp, c_fp]),
    "vilco_nms_workspace": (sz, [i64, i32]),
    "vilco_nms_1d": (C.c_int, [c_fp, c_fp, c_fp, i32, i64, f32, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_softnms_1d": (C.c_int, [c_fp, c_fp, c_fp, i32, i64, f32, f32, f32, i32, i64, c_fp, c_fp, c_fp,
                                   c_fp, sz, c_fp]),
    "vilco_nms_set_kernel": (C.c_int, [i32]),
    "vilco_nms_last_kernels": (C.c_int, []),
    "vilco_det_ap_workspace": (sz, [i64, i32, i32]),
    "vilco_det_ap": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, i64, c_fp, c_fp, c_fp, c_fp, c_fp, i32, i32, c_fp, i32, i32,
                               C.POINTER(C.c_double), i32, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_retrieval_hits_workspace": (sz, [i32, i32, i32]),
    "vilco_retrieval_hits": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, i32, C.POINTER(C.c_double), i32,
                                       C.POINTER(i32), i32, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_score_fuse_workspace": (sz, [i64, i32]),
    "vilco_score_fuse": (C.c_int, [c_fp, c_fp, c_fp, C.POINTER(i32), i64, i32, c_fp, i32, i32, i32, C.POINTER(i32), i64,
                                   c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_nlq_recall_workspace": (sz, [i64, i32]),
    "vilco_nlq_recall": (C.c_int, [c_fp, i32, c_fp, i32, c_fp, c_fp, i64, i32, C.POINTER(C.c_double), i32, C.POINTER(i32), i32,
                                   i32, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_nlq_ensemble": (C.c_int, [c_fp, i32, c_fp, i32, i64, i32, i32, i32, C.c_double, C.c_double, i32, i32, c_fp, c_fp,
                                     c_fp, c_fp, c_fp]),
    "vilco_frob_scale_workspace": (sz, [i64, i64]),
    "vilco_frob_scale": (C.c_int, [c_fp, i64, i64, i64, c_fp, c_fp, sz, c_fp]),
    "vilco_gram_workspace": (sz, [i64, i64]),
    "vilco_gram": (C.c_int, [c_fp, i64, i64, i64, c_fp, c_fp, i32, c_fp, sz, c_fp]),
    "vilco_herd_select_workspace": (sz, [i32, i32, i32]),
    "vilco_herd_select": (C.c_int, [c_fp, i32, i32, i32, i32, c_fp, c_fp, sz, c_fp]),
    "vilco_bic_fit_ws_bytes": (sz, [i64, i32, i32, i32, i32]),
    "vilco_bic_fit": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, i64, i32, c_fp, i32, i32, i32, i32, i32, f32, C.c_double, c_fp,
                                c_fp, c_fp, sz, c_fp]),
    "vilco_bic_eval_ws_bytes": (sz, [i64, i32, i32, i32]),
    "vilco_bic_eval": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, i64, i32, i32, i32, i32, f32, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_bic_correct_fwd": (C.c_int, [C.POINTER(BicCorrectDesc), c_fp]),
    "vilco_bic_correct_bwd_workspace": (sz, [i64]),
    "vilco_bic_correct_bwd": (C.c_int, [C.POINTER(BicCorrectDesc), c_fp, i32, c_fp, c_fp, sz, c_fp]),
    "vilco_ssl_pool_workspace": (sz, [C.POINTER(i32), i32, i32, i32]),
    "vilco_ssl_pool_fwd": (C.c_int, [C.POINTER(c_fp), C.POINTER(i32), i32, c_fp, i32, i32, c_fp, c_fp, sz, c_fp]),
    "vilco_ssl_pool_bwd": (C.c_int, [c_fp, C.POINTER(c_fp), C.POINTER(i32), i32, c_fp, i32, i32, c_fp]),
    "vilco_ssl_nce_workspace": (sz, [i32, i32, i32]),
    "vilco_ssl_nce_fwd": (C.c_int, [c_fp, c_fp, c_fp, i32, i32, c_fp, i32, c_fp, f32, c_fp, c_fp, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_ssl_nce_bwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, i32, i32, i32, f32, c_fp, c_fp, c_fp, sz, c_fp]),
    "vilco_ssl_ring_update": (C.c_int, [c_fp, c_fp, i32, i32, c_fp, i32, c_fp, c_fp]),
    "vilco_prompt_workspace": (sz, [C.POINTER(PromptDesc)]),
    "vilco_prompt_fwd": (C.c_int, [C.POINTER(PromptDesc), c_fp]),
    "vilco_prompt_bwd": (C.c_int, [C.POINTER(PromptDesc), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
    "vilco_status_word_take": (C.c_int, [C.POINTER(i32)]),
    "vilco_coda_workspace": (sz, [C.POINTER(CodaDesc)]),
    "vilco_coda_fwd": (C.c_int, [C.POINTER(CodaDesc), c_fp]),
    "vilco_coda_bwd": (C.c_int, [C.POINTER(CodaDesc), c_fp, c_fp, c_fp, c_fp, c_fp, c_fp]),
}

_lib = None


def load():
    """Load libvilco_hip.so (once).  Raises if it has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libvilco_hip.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C vilco_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise RuntimeError(load().vilco_status_str(int(rc)).decode())


def version():
    return load().vilco_version().decode()
