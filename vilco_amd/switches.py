"""The list of record of the VILCO_* environment variables and of the module-level switches that have none.

One row of `TABLE` per switch: the variable, its default (a string), who reads it (a Python attribute
path, or the file under csrc/ for what only libvilco_hip.so reads), whether `ops.arithmetic_key()` carries it, and one line
of meaning.  The long explanations stay where a switch is used.  Python reads a variable through `on` / `text` / `number`
and nowhere else, at the moment the reading site always did (import, construction or call); the library reads its own
through vilco_env_flag / vilco_env_int (csrc/common.h).  tests/test_switches_cpu.py holds this table against the sources
and the documents.

Imports neither torch nor the library binding.
"""
import os
from collections import namedtuple

Switch = namedtuple("Switch", "env default readers key meaning")

# `key`: KEYED, or why a flip cannot make graph.GraphedStep replay a step recorded under the other setting
KEYED = "keyed"                 # an `ops` attribute that decides which kernels a step records: part of ops.arithmetic_key()
VIA_SET = "ops.set_precision moves ops._precision, which is keyed"
ONCE = "read once per process"
GEN = "read once per process; its setter bumps vilco_gemm_config_gen(), which is part of ops.arithmetic_key()"
BUILT = "read at construction and fixed in the object"
INFERENCE = "inference only"
HOST = "host scheduling only"
PENDING = "unkeyed as before although a flip changes what LayerNorm / attention forward record: to be keyed in a follow-up"

TABLE = (
    # ---- ops.py
    Switch("VILCO_PRECISION", "f16x2", ("ops.DEFAULT_PRECISION",), VIA_SET, "operand format of the matrix products"),
    Switch("VILCO_DW_PRECISION", "f16x1", ("ops.dw_precision",), KEYED, "long weight-gradient products read the leading fp16 part only"),
    Switch("VILCO_GRAPH_STREAMS", "text,heads", ("ops._FORKS",), KEYED, "chains forked onto side streams inside a captured step"),
    Switch("VILCO_DW_FORK_ROWS", "0", ("ops._dw_fork_rows",), KEYED, "with 'dw' forked: only products over at most this many token rows"),
    Switch("VILCO_DEFER_FINISH", "1", ("ops.defer_finish",), KEYED, "second stages of backward's reductions issued together at its end"),
    Switch("VILCO_RANGE_CHECK", "0", ("ops.range_check",), KEYED, "warn | auto: measure the row spread of every Linear backward's dZ"),
    Switch("VILCO_PRODUCER_AMAX", "1", ("ops.produce_amax",), KEYED, "producers leave max|x| partials for the operand packs"),
    Switch("VILCO_PACK_CACHE", "1", ("ops._pack_cache",), PENDING, "an activation's operand planes are remembered on the tensor"),
    Switch("VILCO_PACK_GROUP", "1", ("ops.pack_group_enabled",), KEYED, "the packs of a grouped q / k / v projection as one launch"),
    Switch("VILCO_LN_BWD_AMAX", "1", ("ops.ln_bwd_amax",), KEYED, "LayerNorm backward leaves max|dx| partials"),
    Switch("VILCO_CONV_DZ_PLANES", "1", ("ops.conv_dz_planes",), KEYED, "masked k=3 convs: dZ's operand image from the mask kernel"),
    Switch("VILCO_PACK_REUSE", "1", ("ops._reuse_packs",), KEYED, "one pack of a tensor serves forward, dX and dW"),
    Switch("VILCO_CONV_TAP_PLANES", "1", ("ops.conv_tap_planes",), KEYED, "k=3 convs: x and dZ packed once each for all three products"),
    Switch("VILCO_CONV_DW_KM", "1", ("ops.conv_tap_planes", "gemm.hip"), KEYED, "... and their weight gradient reads those images k-major"),
    Switch("VILCO_WEIGHT_CACHE", "1", ("ops._weight_cache",), KEYED, "weight operand planes kept per parameter version"),
    Switch("VILCO_PRODUCER_PLANES", "1", ("ops.producer_planes",), KEYED, "activation backward writes dz as operand planes"),
    Switch("VILCO_LN_PLANES", "1", ("ops.ln_planes",), KEYED, "LayerNorm forward writes its output as operand planes"),
    Switch("VILCO_ATTN_PLANES", "1", ("ops.attn_planes",), KEYED, "hd = 64 attention forward writes its output as operand planes"),
    Switch("VILCO_LINEAR_GROUP", "1", ("ops.linear_group_enabled",), KEYED, "q / k / v projections as one grouped GEMM launch"),
    Switch(None, "1", ("ops.use_flash",), KEYED, "fused attention kernels (off: materialised scores)"),
    Switch("VILCO_FOLD_SKIP", "1", ("ops.fold_skip_grads",), KEYED, "skip gradients added inside the LayerNorm backward kernel"),
    Switch("VILCO_XL_DS_PLANES", "1", ("ops.xl_ds_planes",), KEYED, "XLNet backward: dS as operand planes from the dQ kernel"),
    Switch("VILCO_XL_SCORES", "1", ("ops.xl_scores_kernel",), KEYED, "XLNet forward: position scores by their own kernel"),
    Switch("VILCO_FUSED_PROMPT", "1", ("ops.fused_prompt",), KEYED, "L2P prompt pool: match, vote and prepend kernels"),
    Switch("VILCO_QKV_PRE", "1", ("ops.use_qkv_pre",), KEYED, "fused ln1 -> depthwise convs -> LayerNorms kernel in MaskedMHCA"),
    # ---- the rest of the Python side
    Switch("VILCO_HIP_LIB", "", ("_lib.LIB_PATH",), ONCE, "library to load instead of vilco_amd/libvilco_hip.so"),
    Switch("VILCO_DP_REPLAY_SYNC", "1", ("graph._DP_REPLAY_SYNC",), HOST, "data-parallel replays wait for the graph before a CPU-side exchange"),
    Switch("VILCO_GRAPH_OWN_STREAM", "1", ("graph._OWN_STREAM",), HOST, "replays leave the default stream for a created one"),
    Switch("VILCO_GRAPH_SHARED_STREAM", "1", ("graph._SHARED_STREAM",), HOST, "... shared by every GraphedStep of the process"),
    Switch("VILCO_DP_SEGMENTS", "1", ("graph._DP_SEGMENTS",), BUILT, "data-parallel backward captured as one graph per stage"),
    Switch("VILCO_DP_GRAPH_COMM", "0", ("graph.GraphedStep.comm_in_graph",), BUILT, "1: the all-reduces captured inside the graph"),
    Switch("VILCO_OPT_AMAX", "1", ("utils.train_utils.OPT_AMAX",), ONCE, "the optimizer update leaves max|w| per chunk for the weight packs"),
    Switch("VILCO_CA_WIDE", "qkv,core,proj", ("modeling.blocks.ChannelAttention.WIDE_PARTS",), ONCE, "channel-attention parts run in bf16 x3"),
    Switch("VILCO_XLNET_CONFIG_DIR", "", ("modeling.backbones._find_xlnet_config",), BUILT, "where xlnet_config_<D>.json is looked for first"),
    Switch("VILCO_HEAD_ROWMASK", "1", ("modeling.meta_archs._HEAD_ROWMASK",), ONCE, "the heads' validity mask applied in the GEMM epilogue"),
    Switch("VILCO_LEVEL_CAT", "1", ("PtTransformer.level_cat",), BUILT, "both heads run over all pyramid levels at once"),
    Switch("VILCO_SYNC_FREE_LOSS", "1", ("PtTransformer.sync_free_loss",), BUILT, "dense, host-sync-free evaluation of the losses"),
    Switch("VILCO_FUSED_LOSS", "1", ("PtTransformer.fused_loss",), BUILT, "ops.mq_loss kernels (0: tensor expressions)"),
    Switch("VILCO_FUSED_SSL", "1", ("PtTransformer.fused_ssl",), BUILT, "ops.ssl_pool / ssl_nce kernels (0: tensor expressions)"),
    Switch("VILCO_DEVICE_DECODE", "1", ("PtTransformer.inference_single_video",), INFERENCE, "vilco_decode (0: the tensor-expression decode)"),
    # ---- read by libvilco_hip.so alone
    Switch("VILCO_ATTN_FAST", "1", ("attn.hip",), ONCE, "hd = 64 attention fast-path kernels"),
    Switch("VILCO_ATTN_XL_FAST", "1", ("attn.hip",), ONCE, "XLNet's relative attention on the hd = 64 fast-path kernels"),
    Switch("VILCO_LAB_ATTN_LDS", "", ("attn.hip",), ONCE, "-DVILCO_LAB_ATTN builds only: the attention kernels' LDS request"),
    Switch("VILCO_GEMM_KM", "1", ("gemm.hip",), ONCE, "transposed operands read k-major from natural-layout planes"),
    Switch("VILCO_GEMM_K2", "1", ("gemm.hip",), ONCE, "single-part products cover two K-steps per barrier interval"),
    Switch("VILCO_GEMM_SUB192", "1", ("gemm.hip",), ONCE, "the two sub-round 192-row plans"),
    Switch("VILCO_GEMM_DW_TALL", "1", ("gemm.hip",), ONCE, "single-part weight-gradient products planned on 192- / 256-row tiles"),
    Switch("VILCO_GEMM_GROUP", "1", ("gemm.hip",), ONCE, "grouped GEMM launches"),
    Switch("VILCO_GEMM_GROUP_DW", "1", ("gemm.hip",), GEN, "initial vilco_gemm_set_group_dw: a backward's equal single-part weight gradients as one launch"),
    Switch("VILCO_GEMM_SKINNY", "1", ("gemm.hip",), ONCE, "initial vilco_gemm_set_skinny: skinny NT products on small workgroups"),
    Switch("VILCO_GEMM_SKINNY_M", "640", ("gemm.hip",), ONCE, "largest M of a skinny product"),
    Switch("VILCO_GEMM_SKINNY_BM16", "640", ("gemm.hip",), ONCE, "largest M on 16-row workgroups"),
    Switch("VILCO_GEMM_SKINNY_K", "768", ("gemm.hip",), ONCE, "largest K of a skinny product"),
    Switch("VILCO_GEMM_BM", "0", ("gemm.hip",), ONCE, "initial vilco_gemm_force: tile height"),
    Switch("VILCO_GEMM_KS", "0", ("gemm.hip",), ONCE, "initial vilco_gemm_force: split-K count"),
    Switch("VILCO_ACT_BWD_VEC", "1", ("eltwise.hip",), ONCE, "four channels per thread in the activation-backward kernel"),
    Switch("VILCO_QKV_TB", "0", ("qkvpre.hip",), ONCE, "forced tokens per workgroup of the three-pass q/k/v pre-projection"),
    Switch("VILCO_QKV_RING", "-1", ("qkvpre.hip",), ONCE, "1 / 0: the ring form of the q/k/v pre-projection always / never"),
    Switch("VILCO_PACK_CAP", "768", ("pack.h",), ONCE, "workgroup cap of the natural-layout pack kernel"),
    Switch("VILCO_SOFTNMS_LEGACY", "0", ("nms.hip",), ONCE, "initial vilco_nms_set_kernel: 1 = one pass per pick only"),
    Switch("VILCO_SOFTNMS_REG", "1", ("nms.hip",), ONCE, "initial vilco_nms_set_kernel: 0 = nothing faster than the row-strided kernel"),
)

_DEFAULT = {s.env: s.default for s in TABLE if s.env is not None}
# attribute names of `ops` that make up ops.arithmetic_key(), in table order
KEYED_OPS = tuple(dict.fromkeys(r[4:] for s in TABLE if s.key == KEYED for r in s.readers if r.startswith("ops.")))


def text(env):
    """the variable's value now, or its declared default (KeyError: not in TABLE)"""
    return os.environ.get(env, _DEFAULT[env])


def on(env):
    """a flag: everything but "0" is on"""
    return text(env) != "0"


def number(env):
    return int(text(env))
