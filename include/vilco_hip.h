/*
 * vilco_hip.h -- C ABI of libvilco_hip.so, the MI355X (gfx950) kernel library behind the
 * drop-in MQ modules in vilco_amd/modeling.
 *
 * The reference (cruiseresearchgroup/ViLCo, MQ tree) has no C operator API for this path: its
 * operators are torch.nn.functional calls inside MQ/libs/modeling (python) plus ONE compiled
 * extension, nms_1d_cpu (MQ/libs/utils/csrc/nms_cpu.cpp:172-182).  Each entry point below cites
 * the reference code whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer owned by the caller
 *    (PyTorch caching allocator) unless stated; `stream` is a hipStream_t passed as void*.
 *  - activations are TOKEN-MAJOR fp32: x[b][t][c] (c contiguous) -- the reference is channel-first
 *    [B,C,T] (blocks.py:107-108); vilco_transpose2d converts at the module boundary.
 *  - sequence masks are prefix masks (meta_archs.py:1175 `arange < len`), passed as int32 len[B].
 *  - functions never allocate, never synchronise, never throw; they return 0 or a negative status.
 */
#ifndef VILCO_HIP_H
#define VILCO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vilco_status {
  VILCO_OK = 0,
  VILCO_ERR_BADARG = -1,      /* null pointer / negative size / misaligned operand */
  VILCO_ERR_UNSUPPORTED = -2, /* shape outside what the kernels implement */
  VILCO_ERR_LAUNCH = -3,      /* hipLaunchKernel reported an error */
  VILCO_ERR_WORKSPACE = -4    /* workspace too small */
};

const char* vilco_status_str(int status);
/* library / target identification: "vilco_hip <ver> gfx950" */
const char* vilco_version(void);
/* sizeof of a struct of this header by its name ("vilco_gemm_desc", ...), 0 for an unknown name: lets a binding check its mirror */
size_t vilco_abi_sizeof(const char* struct_name);

/* ------------------------------------------------------------------------------------------ */
/* GEMM family: every 1x1 conv, k=3 conv, nn.Linear, einsum projection and (round 1) the        */
/* attention contractions.  C[m][n] = epilogue(alpha * sum_k A(m,k) B(k,n)).                    */
/* Replaces aten::convolution / addmm / bmm / einsum under blocks.py:79,217-226,340-349,420-435, */
/* 533-539, meta_archs.py:216-235,309-331, modeling_xlnet_x.py:284-325,437-443,474-489.         */
/* Operands are split once into 16-bit planes in their natural row-major layout (vilco_pack; the same planes serve    */
/* the k-contiguous and the k-major use, the latter through transposing LDS reads), then ONE MFMA kernel runs on the  */
/* planes: 256 / 192 / 128 x 128 x 32 tiles chosen per problem, 8 waves in a ping-pong schedule, optional split-K.    */
/* Default precision 3: two fp16 parts of operands scaled by a per-tensor power of two (v_mfma_f32_16x16x32_f16,     */
/* 3 MFMAs per product, ~2^-22, fp32 accumulate).  Others: 0 = split-bf16 (hi+lo, 3 MFMAs, ~2^-17 relative),           */
/* 1 = single bf16 pass, 2 = three-part bf16 split (6 MFMAs, ~2^-25: numerically an fp32 GEMM, 8 exponent bits per    */
/* element -- the format of call sites whose tensors span too much range for one scale);  4 = the fp16 x2 planes, but the */
/* product takes their leading parts only (1 MFMA, 11-bit operands, fp32 accumulate): for the weight-  */
/* gradient products dW = dY^T X, whose rounding errors average over the B*T contraction and feed   */
/* nothing downstream (ops.py: dw_precision).                                                        */
/* ------------------------------------------------------------------------------------------ */
enum { VILCO_ACT_NONE = 0, VILCO_ACT_RELU = 1, VILCO_ACT_GELU = 2 };
enum { VILCO_TAP_NONE = 0, VILCO_TAP_A = 1, VILCO_TAP_B = 2 };

typedef struct vilco_gemm_desc {
  const float* A;
  const float* B;
  float* C;
  int32_t M, N, K;
  int32_t a_kcontig; /* 1: A(m,k) = A[m*lda + k];  0: A(m,k) = A[k*lda + m] */
  int32_t b_kcontig; /* 1: B(k,n) = B[n*ldb + k];  0: B(k,n) = B[k*ldb + n] */
  int64_t lda, ldb, ldc;
  /* batch z = zo*batch_inner + zi ; pointer offset = zo*s?o + zi*s?i (elements) */
  int32_t batch_outer, batch_inner;
  int64_t sAo, sAi, sBo, sBi, sCo, sCi;
  /* k=3 "same" conv as a GEMM over overlapped token rows (MaskedConv1D, blocks.py:79,114):
   * the tapped operand's contiguous dim spans 3*tapC (taps t-1,t,t+1), its row index is a token
   * (b*tapT + t); element address = base + row*ld + col - tapC, zero outside [0,tapT). */
  int32_t tap_operand, tapC, tapT;
  int32_t precision;
  float alpha, beta; /* result += beta * C_old (after the whole epilogue) */
  /* epilogue, applied in this order; each optional (null / 0 = off) */
  const float* bias;      /* [N]                                       */
  float* preact;          /* same layout as C: value before activation */
  int32_t act;            /* VILCO_ACT_*                               */
  const int32_t* row_len; /* row m -> b = m / rowT, t = m % rowT; zero the row when t >= row_len[b] */
  int32_t rowT;
  const float* colscale;  /* [N]  (AffineDropPath.scale, blocks.py:663-670) */
  const float* residual;  /* same layout as C; added after scaling */
  int32_t res_masked;     /* 1: residual is also zeroed on masked rows */
  /* device scratch for the bf16 operand planes and split-K partials; size from vilco_gemm_workspace() */
  void* workspace;
  size_t workspace_bytes;
  /* optional operands already packed by vilco_pack (NULL: the call packs A / B itself).  The packed tensor is the  */
  /* row-major matrix the operand lives in: [M][K] (a_kcontig = 1) or [K][M] (a_kcontig = 0), likewise [N][K] /    */
  /* [K][N] for B -- ONE pack of an activation, a weight or an output gradient serves every product it appears in  */
  /* (forward, dX = dY W and dW = dY^T X).  For tap_operand = NONE and batch 1 (A / B may then be NULL), and for    */
  /* the weight operand B ([N][3*tapC], k-contiguous) of a conv whose taps are on A (tap_operand = TAP_A).          */
  const void* a_planes;
  const void* b_planes;
  /* XLNet relative-position band (modeling_xlnet_x.py:204-214, 284-325): with T = bandT only the entries          */
  /* 0 <= p - T + i < T of the [T, 2T] position-score matrix (row i, column p) are ever used / non-zero.            */
  /*   band 1: C is that matrix (M = T rows i, N = 2T columns p): output tiles wholly outside the band are skipped  */
  /*           (left unwritten);  band 2: A is that matrix, k = p (M rows i): K-steps outside a tile's band are     */
  /*           skipped;  band 3: A is its transpose, M rows p, k = i: likewise.  0: dense.                          */
  int32_t band, bandT;
  /* fused inverted dropout on the stored output (after activation, row mask, column scale; before residual / beta):   */
  /* the mask of vilco_dropout(p, seed) at element index m*N + n.  Needs ldc == N, batch 1.  0: none.                     */
  float drop_p;
  uint32_t drop_seed;
  /* optional: the call leaves vilco_gemm_amax_parts(desc) partial maxima of |C| (as stored, after the whole epilogue)  */
  /* here -- one per workgroup of the kernel that writes C -- for the operand pack of the next product                  */
  /* (vilco_pack_item.amax), which then needs no pass of its own over C.  NULL: not wanted.                             */
  float* amax_out;
  /* optional (precision 3, operands the call packs itself -- A / B given as fp32): max|x| partials of the WHOLE operand  */
  /* tensor already on the device, left by the kernel that produced it; the call then skips its amax pass over it.      */
  const float* a_amax; int32_t a_namax;
  const float* b_amax; int32_t b_namax;
  /* 1: a_planes / b_planes hold the k=3 convs' zero-padded per-sequence image (vilco_pack_item.seq_len = tapT) instead of */
  /* the natural [rows32][cols32] layout.  Required for -- and only legal with -- the tapped operand of a conv product:     */
  /* tap_operand = TAP_A: a_planes (tapC % 8 == 0);  TAP_B (the weight gradient, M % 8 == 0, tapC % 8 == 0): BOTH operands, */
  /* a_planes = the image of dZ [K rows of width M], b_planes = the image of the conv input [K rows of width tapC].          */
  int32_t a_planes_seq, b_planes_seq;
  /* optional: one float per output row m (M floats, one batch element only): rows with row_mask[m] == 0 are zeroed exactly as */
  /* rows beyond row_len are -- a validity pattern that is not "the first len rows of every sequence" (the heads over the        */
  /* concatenated pyramid levels: per level, per clip; meta_archs.py:216-235 applies mask[level] after every conv)               */
  const float* row_mask;
} vilco_gemm_desc;

size_t vilco_gemm_workspace(const vilco_gemm_desc* d);
int vilco_gemm(const vilco_gemm_desc* d, void* stream);
/* n (1..4) INDEPENDENT products of one shape / orientation / format as ONE launch (round 5: the q / k / v projections of an
 * attention block -- MQ/libs/modeling/blocks.py:332-344 -- forward and dX; each alone is a 75 %-full round of tiles on 256 CUs).
 * Requires packed operands (a_planes / b_planes), precision 3, no batch / tap / band, equal M, N, K and orientations, and a
 * plan without split-K; anything else runs as n vilco_gemm calls in order.  Same arithmetic either way.  VILCO_GEMM_GROUP=0:
 * always ungrouped. */
int vilco_gemm_group(const vilco_gemm_desc* descs, int32_t n, void* stream);
/* Precision 4 (the single-part weight gradients dW = dZ^T X; reference: autograd's weight gradient of every nn.Linear / 1x1
 * MaskedConv1D of blocks.py) is grouped too, for any n >= 2: equal products with packed operands and the plain epilogue (alpha 1,
 * beta 0, nothing fused), no batch / tap / band, nothing forced by vilco_gemm_force, run as one gemm_pp_group_kernel launch per
 * 16 products -- n x tiles >= 256 workgroups: no split-K, each dW written once; fewer: the smallest split count that fills one
 * round of the chip.  One pass over K per output element instead of one per slab: same products, another summation order than
 * the split plan of a lone launch (bit-equal to a lone launch with one split).  Every member's workspace must hold
 * vilco_gemm_group_workspace(member, n) bytes.  VILCO_GEMM_GROUP_DW=0 (or a group the plan prices above its members): n
 * vilco_gemm calls in order. */
size_t vilco_gemm_group_workspace(const vilco_gemm_desc* d, int32_t n);
/* the switch of the precision-4 groups (initial value: environment VILCO_GEMM_GROUP_DW, default 1) and its current value; the
 * setter bumps vilco_gemm_config_gen(): the summation order of the grouped weight gradients differs from the split plans'. */
int vilco_gemm_set_group_dw(int32_t on);
int32_t vilco_gemm_group_dw(void);

/* Timing of the MFMA kernel alone (not the packs, not the split-K reduce): between begin and end every vilco_gemm   */
/* brackets its main kernel with HIP events on the caller's stream; end waits for them and returns the sum.          */
/* Tuning override: force the tile height (128 | 192 | 256; 0 = cost model) and split-K count (0 = heuristic) of every
 * following vilco_gemm in this process.  Initial values: environment VILCO_GEMM_BM / VILCO_GEMM_KS, read once. */
int vilco_gemm_force(int32_t bm, int32_t ks);
/* Round 6: few-row NT products of the default precision (M <= 640 token rows: the pyramid levels at T' <= 288, the 77 text tokens, every
 * level of BASELINE configs[0]; reference: the nn.Linear / 1x1 MaskedConv1D calls of blocks.py:191-269 at those levels) run as ONE
 * launch of gemm_skinny_kernel (the eight waves of a workgroup split K, fragments straight from the operand planes, partial tiles
 * summed through LDS) instead of a split-K plan of the tiled kernel + its reduce launch.  1 (default) / 0; env VILCO_GEMM_SKINNY,
 * VILCO_GEMM_SKINNY_M = the largest M that takes it (640).  Same arithmetic per product (two fp16 parts, three MFMAs, fp32
 * accumulation); the summation order over K differs from the tiled kernels'. */
int vilco_gemm_set_skinny(int32_t on);
/* Generation of the process-wide GEMM configuration: bumped by vilco_gemm_force / vilco_gemm_set_skinny.  The host
 * side keys captured hipGraphs on it (a replay runs the plan that was recorded, not the current configuration). */
int64_t vilco_gemm_config_gen(void);
/* floats written to desc->amax_out by vilco_gemm(desc) (depends on the tile / split-K plan); 0: not available */
int32_t vilco_gemm_amax_parts(const vilco_gemm_desc* desc);
int vilco_gemm_profile_begin(void);
int vilco_gemm_profile_end(double* kernel_ms, int64_t* launches);
/* per-launch records of the last begin/end bracket (measurement tooling, tools/gemm_shapes.py): desc[i*10 + 0..9] =
 * M, N, K, batch, tile rows, split-K count, precision, a k-major, b k-major, tap flags; ms[i] = that launch's kernel
 * time.  Returns the number of records available (may exceed cap). */
int64_t vilco_gemm_profile_records(int64_t* desc, double* ms, int64_t cap);

/* Splits the fp32 row-major matrix src[rows][cols] (row stride ld) ONCE into the 16-bit operand planes of         */
/* `precision` ([part][rows32][cols32], zero padded; precision 3 also leaves the per-tensor power-of-two scale in  */
/* the buffer's header).  `planes` is device memory, 256-byte aligned, vilco_pack_bytes() long.                     */
size_t vilco_pack_bytes(int64_t rows, int64_t cols, int32_t precision);
int vilco_pack(const float* src, int64_t rows, int64_t cols, int64_t ld, int32_t precision, void* planes,
               size_t planes_bytes, void* stream);
/* up to four tensors in the same two launches (an activation and its layer's weight) */
typedef struct vilco_pack_item {
  const float* src;
  int64_t rows, cols, ld;
  void* planes;
  size_t planes_bytes;
  /* optional: `nbatch` matrices `batch_stride` floats apart (0 / 1 = one matrix); the planes are then            */
  /* [part][batch][rows32][cols32] and serve batched vilco_gemm calls whose A / B batches are numbered the same   */
  int32_t nbatch;
  int64_t batch_stride;
  /* relshift = 1: pack XLNet's unshifted view [rows][rows + cols] of src[rows][cols] (element (i,p) =            */
  /* src[i][p - rows + i] or 0): the adjoint of rel_shift_bnij, so dS feeds the position-term gradients directly  */
  int32_t relshift;
  /* optional (precision 3): `namax` partial maxima of |src| already on the device -- left by the kernel that produced  */
  /* src (vilco_layernorm_fwd, vilco_act_bwd, vilco_qkv_pre_fwd: their amax_parts) -- so the pack needs no amax launch  */
  const float* amax;
  int32_t namax;
  /* seq_len = T > 0: src is rows / T token sequences of T rows (cols % 8 == 0) and the planes are the image the k=3 convs   */
  /* read -- every sequence with one zero row before and after it, [nseq * (T + 2) + zero rows][cols], no column padding:    */
  /* ONE pack of a conv's input x serves the forward product (vilco_gemm, tap_operand = TAP_A, a_planes) and the weight     */
  /* gradient (TAP_B, b_planes); one pack of dZ serves dX (TAP_A) and the weight gradient (TAP_B, a_planes).                 */
  /* Reference: the im2col-free form of F.conv1d under MaskedConv1D, blocks.py:106-130.                                      */
  int32_t seq_len;
} vilco_pack_item;
size_t vilco_pack_item_bytes(const vilco_pack_item* item, int32_t precision);   /* honours nbatch / relshift */
int vilco_pack_many(const vilco_pack_item* items, int32_t n, int32_t precision, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* LayerNorm over the channel dim of token-major rows: blocks.py:160-175 (biased variance, eps   */
/* inside sqrt) and the stock nn.LayerNorm calls (blocks.py:446-451, modeling_xlnet_x.py:236,473). */
/* relu=1 fuses the ReLU that follows every embed/head LN (backbones.py:219, meta_archs.py:270).  */
/* ------------------------------------------------------------------------------------------ */
/* Forward.  Zero-initialise, set what the call uses; a null / 0 field = that part off. */
typedef struct vilco_ln_fwd_desc {
  const float* x;        /* [rows][C] */
  const float* gamma;    /* [C] or NULL */
  const float* beta;     /* [C] or NULL */
  float* y;              /* [rows][C] */
  float* mean;           /* [rows], kept for backward; NULL: not wanted */
  float* rstd;           /* [rows], likewise */
  int64_t rows;
  int32_t C;
  float eps;
  int32_t relu;
  /* optional: the kernel also leaves *n_parts per-block partial maxima of |y| in amax_parts (device, >= 2048 floats): the operand */
  /* pack of y (vilco_pack_item.amax) then needs no separate pass over it.  n_parts: HOST int32, written by the call.              */
  float* amax_parts;
  int32_t* n_parts;
  /* optional: y also written by the kernel as the fp16 x2 operand planes (precision 3) of the product that consumes it:           */
  /* seq_len = 0: vilco_pack's layout for [rows][C] (C % 32 == 0); seq_len = T > 0: the k=3 convs' zero-padded per-sequence image   */
  /* (vilco_pack_item.seq_len; C % 8 == 0, rows % T == 0).  `planes`: device, 256-byte aligned, vilco_layernorm_planes_bytes() long */
  /* (= vilco_pack_bytes / vilco_pack_item_bytes of the same tensor).  The planes' scale comes from the bound                       */
  /* max|gamma| sqrt(C) + max|beta| >= max|y| instead of the exact maximum: no pass over y, no pack launch.                         */
  void* planes;
  size_t planes_bytes;
  int32_t seq_len;
  /* optional (with or without planes): y[row][:] *= row_mask[row % mask_rows] -- the zero separator rows of the heads' concatenated */
  /* pyramid levels (meta_archs.py:216-235 runs the shared head per level); with relu = 1 and a 0 / 1 mask vilco_layernorm_bwd needs  */
  /* no mask of its own: it already drops the gradient wherever the saved y is 0.                                                     */
  const float* row_mask;
  int64_t mask_rows;
} vilco_ln_fwd_desc;
size_t vilco_layernorm_planes_bytes(int64_t rows, int32_t C, int32_t seq_len);
int vilco_layernorm_fwd(const vilco_ln_fwd_desc* d, void* stream);

typedef struct vilco_ln_bwd_desc {
  const float* dy;       /* [rows][C] */
  const float* x;
  const float* y;        /* forward output: only read when relu = 1 */
  const float* gamma;
  const float* mean;
  const float* rstd;
  /* optional ([rows][C]): dx = LayerNorm backward + dres -- the gradient that reaches x over the residual connection around the   */
  /* branch this LayerNorm opens (blocks.py:571-590: x + drop_path(attn(ln1(x))), out + drop_path(mlp(ln2(out)))): the sum         */
  /* autograd would form with a kernel of its own.                                                                                 */
  const float* dres;
  float* dx;
  float* dgamma;         /* [C], overwritten; dgamma and dbeta both set or both NULL */
  float* dbeta;
  int64_t rows;
  int32_t C;
  int32_t relu;
  void* workspace;       /* vilco_layernorm_bwd_workspace() bytes */
  size_t workspace_bytes;
  /* optional (round 6): partial maxima of |dx| (device, >= 2048 floats; *n_parts, HOST int32 = how many were written): dx is the  */
  /* output gradient of the layer in front of the LayerNorm, whose mask / activation-backward kernel turns it into operand planes   */
  /* (vilco_act_bwd_desc.planes) from that bound.                                                                                   */
  float* dx_amax_parts;
  int32_t* n_parts;
} vilco_ln_bwd_desc;
size_t vilco_layernorm_bwd_workspace(int64_t rows, int32_t C);
int vilco_layernorm_bwd(const vilco_ln_bwd_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Depthwise k=3 conv, stride 1|2, zero pad 1, no bias, output masked: MaskedMHCA's query/key/   */
/* value convs (blocks.py:312-334,363-368 via MaskedConv1D.forward :106-130).                    */
/* x[B][Tin][C], w[C][3], y[B][Tout][C], Tout = Tin/stride, valid(t') = stride*t' < in_len[b].   */
/* ------------------------------------------------------------------------------------------ */
int vilco_dwconv3_fwd(const float* x, const float* w, const int32_t* in_len, float* y, int32_t B,
                      int32_t Tin, int32_t C, int32_t stride, void* stream);
size_t vilco_dwconv3_bwd_workspace(int32_t B, int32_t Tin, int32_t C, int32_t stride);
int vilco_dwconv3_bwd(const float* dy, const float* x, const float* w, const int32_t* in_len,
                      float* dx, float* dw, int32_t B, int32_t Tin, int32_t C, int32_t stride,
                      void* workspace, size_t workspace_bytes, void* stream);

/* nn.MaxPool1d(3, 2, 1) skip path times the output mask (blocks.py:519-523,567). */
int vilco_maxpool3s2_fwd(const float* x, const int32_t* in_len, float* y, int32_t B, int32_t Tin,
                         int32_t C, void* stream);
int vilco_maxpool3s2_bwd(const float* dy, const float* x, const int32_t* in_len, float* dx,
                         int32_t B, int32_t Tin, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Row softmax over materialised attention scores S[B][H][Tq][Tk], in place.                     */
/* mode 0: key j masked (-inf) when j >= kv_len[b]   (blocks.py:258-260, 390-392)                */
/* mode 1: XLNet: score - 1e30 when (j >= kv_len[b] && j != i)  (modeling_xlnet_x.py:1184-1188,  */
/*         298-307); mode 2: no mask (ChannelAttention, blocks.py:432).                          */
/* ------------------------------------------------------------------------------------------ */
int vilco_softmax_fwd(float* s, const int32_t* kv_len, int32_t B, int32_t H, int32_t Tq,
                      int32_t Tk, int32_t mode, void* stream);
/* dS = P * (dP - sum_j dP*P), written over dp */
int vilco_softmax_bwd(float* dp, const float* p, int32_t B, int32_t H, int32_t Tq, int32_t Tk,
                      void* stream);
/* XLNet rel_shift_bnij fused with the add (modeling_xlnet_x.py:256-268,288,298):
 * s[b][h][i][j] += scale * bd[b][h][i][T - i + j],  bd is [B][H][T][2T]. */
int vilco_relshift_add(float* s, const float* bd, float scale, int32_t B, int32_t H, int32_t T,
                       void* stream);
/* adjoint: dbd[b][h][i][T-i+j] = scale * ds[b][h][i][j], all other entries 0 */
int vilco_relshift_bwd(const float* ds, float* dbd, float scale, int32_t B, int32_t H, int32_t T,
                       void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused (flash-style) masked multi-head attention, heads = channel slices of token-major q/k/v:  */
/* MaskedMHCA / MaskedMHA cores (blocks.py:383-400, 251-265) and, with `bias`, XLNet's             */
/* rel_attn_core (modeling_xlnet_x.py:270-320; bias = scale * rel_shift(bd)).  Scores stay on chip. */
/* q [B,Tq,H*hd], k/v [B,Tk,H*hd], bias [B,H,Tq,Tk] or null, lse [B,H,Tq] (saved for backward).     */
/* mask modes as vilco_softmax_fwd (+ 3: XLNet mask with the bias given as unshifted position scores [B,H,Tq,Tq+Tk]; */
/* + 4: sliding window |i - j| <= window below kv_len, Tq == Tk -- NLQ's LocalMaskedMHCA, NLQ/libs/modeling/blocks.py   */
/* :417-755; only the key tiles a query tile's windows reach are visited.  window >= Tk is taken as window = Tk -- every key    */
/* below kv_len, the same for any such value up to INT32_MAX.  A query row with no key left (i - window >= kv_len[b]) gives a */
/* zero row of o and of dq and enters no gradient; kv_len[b] = 0 in this mode gives exact zeros in o, dq, dk and dv of clip b */
/* and nothing else anywhere.  A query row with exactly one key (window 0, a clip of length 1) has the constant softmax 1: */
/* it adds exactly zero to dq and dk, and only to dv);                                                                        */
/* precision as vilco_gemm.  hd <= 160 (<= 64 in bf16 x3), hd % 4 == 0.  drop_p > 0: inverted dropout on the attention probabilities      */
/* (after the softmax, before P V) with a counter-based mask of its own (round 5; vilco_attn_dropout_mask writes it     */
/* out): one strong hash per row bh*Tq + i of stream drop_seed, a two-multiply finalizer per element (row key, j);      */
/* forward and backward must be given the same (drop_p, drop_seed).                                                    */
/* ------------------------------------------------------------------------------------------ */
int vilco_attn_supported(int32_t hd);
/* Output amax partials.  The hd = 64 / fp16 x2 / prefix-mask / no-bias / no-dropout kernels can leave max|x| partials of
 * their outputs (one float per workgroup) for the operand pack of the next product (vilco_pack_item.amax), which then
 * skips its amax launch.  Returns how many floats the o / dq buffer (key_side = 0, T = Tq) or the dk / dv buffers
 * (key_side = 1, T = Tk) must hold, or 0 when this configuration does not emit them (pass null then).  has_bias = 2
 * asks for the dS (dbias) partials of XLNet's relative attention (mask mode 3, Tq = Tk = T, key_side 0: dbias_amax). */
int32_t vilco_attn_amax_parts(int32_t B, int32_t H, int32_t T, int32_t hd, int32_t mode, int32_t precision,
                              int32_t has_bias, float drop_p, int32_t key_side);
/* Input amax partials (precision 3): max|x| partials of q / k / v / dout already on the device, e.g. left by the GEMM   */
/* that produced them (vilco_gemm_desc.amax_out).  A tensor with a NULL pointer or a count of 0 gets its own amax pass. */
typedef struct vilco_attn_amax_in {
  const float* q; int32_t nq;
  const float* k; int32_t nk;
  const float* v; int32_t nv;
  const float* dout; int32_t ndo;       /* backward only */
} vilco_attn_amax_in;
/* One descriptor for both directions (zero-initialise; forward ignores the backward-only fields). */
typedef struct vilco_attn_desc {
  const float* q;        /* [B,Tq,H*hd] */
  const float* k;        /* [B,Tk,H*hd] */
  const float* v;
  const float* bias;     /* [B,H,Tq,Tk] or NULL */
  const int32_t* kv_len; /* [B]; may be NULL in mask mode 2 */
  float* o;              /* forward: output; backward: the forward's output (read) */
  float* lse;            /* [B,H,Tq]: written by forward, read by backward */
  int32_t B, H, Tq, Tk, hd;
  float scale;
  int32_t mode, window, precision;
  float drop_p;
  uint32_t drop_seed;
  const vilco_attn_amax_in* amax_in;   /* may be NULL: see above */
  /* workspace = 16-bit operand planes (q, k natural; v transposed, or natural on the hd = 64 fast path), built inside the call by  */
  /* the pack kernels; vilco_attn_fwd_workspace() / vilco_attn_bwd_workspace() bytes                                                */
  void* workspace;
  size_t workspace_bytes;
  /* forward only */
  float* o_amax;         /* see vilco_attn_amax_parts (NULL = not wanted) */
  /* optional: o also written as the fp16 x2 operand planes (vilco_pack's layout for [B * Tq][H * hd], precision 3, vilco_pack_bytes */
  /* long, 256-byte aligned) of the output projection -- the hd = 64 kernels only (vilco_attn_planes_supported: when                 */
  /* vilco_attn_amax_parts(...) > 0, or XLNet's relative attention at hd = 64).  Scale from the bound max|o| <= max|v| / keep.       */
  void* o_planes;
  size_t o_planes_bytes;
  /* backward only: dq / dk / dv are overwritten; dbias (optional, [B,H,Tq,Tk]) receives dS.  Deterministic (no atomics). */
  const float* dout;
  float* dq;
  float* dk;
  float* dv;
  float* dbias;
  float* dq_amax;        /* see vilco_attn_amax_parts (NULL = not wanted) */
  float* dk_amax;
  float* dv_amax;
  float* dbias_amax;
  /* optional (round 5), XLNet's relative attention (mask mode 3, hd = 64, precision 3, Tq = Tk): the backward writes dS -- the      */
  /* gradient of the position scores, modeling_xlnet_x.py:256-288 -- directly as the fp16 x2 operand planes of the UNSHIFTED          */
  /* [Tq][Tq + Tk] view (the layout vilco_pack_many gives an item with relshift = 1, nbatch = B*H), ready for the two band-limited    */
  /* products d(qr) = d(bd) kr and d(kr) = d(bd)^T qr (vilco_gemm_desc.a_planes, band 2 / 3), instead of fp32 dS + a pack pass        */
  /* (0.68 GB written, 0.68 GB read and 1.36 GB written again at config P).  `ds_planes`: at least vilco_attn_dsplanes_bytes(B, H,    */
  /* Tq) bytes, 256-byte aligned, whose out-of-band columns (p < Tq - i, p >= Tq + Tk - i of row i) and padding are ZERO: the kernel  */
  /* writes the band only, so a buffer zeroed once can be reused call after call.  `dbias` and `dbias_amax` must be NULL with it and  */
  /* Tk a multiple of 64.                                                                                                             */
  void* ds_planes;
  size_t ds_planes_bytes;
} vilco_attn_desc;
size_t vilco_attn_fwd_workspace(int32_t B, int32_t H, int32_t Tq, int32_t Tk, int32_t hd, int32_t precision);
int32_t vilco_attn_planes_supported(int32_t Tq, int32_t Tk, int32_t hd, int32_t mode, int32_t precision, int32_t has_bias,
                                    float drop_p);
int vilco_attn_fwd(const vilco_attn_desc* d, void* stream);
size_t vilco_attn_bwd_workspace(int32_t B, int32_t H, int32_t Tq, int32_t Tk, int32_t hd, int32_t precision);
size_t vilco_attn_dsplanes_bytes(int32_t B, int32_t H, int32_t T);
int vilco_attn_bwd(const vilco_attn_desc* d, void* stream);
/* XLNet's position scores bd[b][h][i][p] = qr[b][i][h] . kr[(b)][p][h] for the band p in [T - i, 2T - i) of the unshifted    */
/* [T][2T] matrix -- the part rel_shift_bnij keeps (modeling_xlnet_x.py:204-214, 256-288); the rest of bd is left unwritten.   */
/* qr [B][T][H*hd], kr [2T][H*hd] (per_clip 0) or [B][2T][H*hd] (per_clip 1: the reference drops out the expanded position     */
/* embedding per batch element), bd [B][H][T][2T] fp32, read in place by vilco_attn_fwd / _bwd (mask mode 3).  hd = 64,       */
/* precision 3 only.  Replaces the band-1 vilco_gemm with K = 64 (write-bound at 1.9 TB/s; this kernel: the attention kernels'  */
/* first product with the qr fragments resident).                                                                             */
size_t vilco_xl_scores_workspace(int32_t B, int32_t H, int32_t T, int32_t per_clip);
int vilco_xl_scores(const float* qr, const float* kr, float* bd, int32_t B, int32_t H, int32_t T, int32_t hd,
                    int32_t per_clip, int32_t precision, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Candidate decode of PtTransformer.inference_single_video (MQ meta_archs.py:1594-1692, NLQ meta_archs.py:1253-1338)   */
/* for ONE clip, all L pyramid levels in one call: per level sigmoid(logit) > pre_nms_thresh on the valid positions,  */
/* the pre_nms_topk highest of those (exact; ties at the cut admitted in index order), segment = (t - off_l * stride,   */
/* t + off_r * stride), kept when longer than duration_thresh.  logits [R][C], offsets [R][2] (the regression head's    */
/* relu(Scale_l(x))), points [R][4] = (t, lo, hi, stride) share one row layout; level l owns rows level_row0[l] ..      */
/* level_row0[l] + level_len[l] - 1 (level_len = valid length of the clip at that level).  Outputs: the candidates of    */
/* level 0, then level 1, ... (inside a level in index order -- every consumer orders by score itself), out_total[0] =   */
/* how many; capacity L * topk rows.  L <= 64.                                                                           */
/* ------------------------------------------------------------------------------------------ */
size_t vilco_decode_workspace(int32_t L, int32_t topk);
int vilco_decode(const float* logits, const float* offsets, const float* points, const int32_t* level_row0,
                 const int32_t* level_len, int32_t C, int32_t L, int32_t topk, float pre_nms_thresh,
                 float duration_thresh, float* out_segs, float* out_scores, int64_t* out_labels,
                 int32_t* out_total, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Elementwise / reduction glue of TransformerBlock.forward (blocks.py:561-593).                 */
/* ------------------------------------------------------------------------------------------ */
/* out = a * (mask_a ? m : 1) + colscale[c] * rowscale[b] * bval ; colscale/rowscale/len optional */
int vilco_scale_add_fwd(float* out, const float* a, const float* bval, const float* colscale,
                        const float* rowscale, const int32_t* len, int32_t mask_a, int32_t B,
                        int32_t T, int32_t C, void* stream);
size_t vilco_colsum_workspace(int64_t rows, int32_t C);
/* da = dout*(mask_a?m:1) ; db = dout*colscale*rowscale ; dcolscale = sum_rows dout*bval*rowscale. */
typedef struct vilco_scale_add_bwd_desc {
  const float* dout;     /* [B][T][C] */
  const float* bval;     /* needed for dcolscale */
  const float* colscale; /* [C] or NULL */
  const float* rowscale; /* [B] or NULL */
  const int32_t* len;    /* [B] or NULL */
  int32_t mask_a;
  float* da;             /* da / db / dcolscale may be NULL to skip */
  float* db;
  float* dcolscale;
  int32_t B, T, C;
  void* workspace;       /* vilco_colsum_workspace(B * T, C) bytes when dcolscale is wanted */
  size_t workspace_bytes;
  /* optional: partial maxima of |db| (device, >= 2048 floats; *n_parts, HOST int32 = how many were written): db is the upstream    */
  /* gradient of the residual branch's last layer, whose activation-backward kernel turns it into operand planes                     */
  /* (vilco_act_bwd_desc.planes)                                                                                                     */
  float* db_amax_parts;
  int32_t* n_parts;
} vilco_scale_add_bwd_desc;
int vilco_scale_add_bwd(const vilco_scale_add_bwd_desc* d, void* stream);
/* Inverted dropout y = keep ? x/(1-p) : 0 with a counter-based mask (element i of the stream `seed` at `offset + i`):   */
/* the backward pass is the same call on dy.  x = NULL writes the mask factors (0 or 1/(1-p)) -- what the parity tests  */
/* hand to the oracle.  nn.Dropout in modeling_xlnet_x.py:308,327,486,488,1201,1228,1280 and blocks.py:226,268,349.      */
int vilco_dropout(const float* x, float* y, int64_t n, float p, uint32_t seed, uint64_t offset, void* stream);
/* The mask factors (0 or 1/(1-p)) vilco_attn_fwd / vilco_attn_bwd apply to the attention probabilities under (p, seed):  */
/* y[rows = B*H*Tq][cols = Tk].  For tests and for replaying a step's masks in the CPU oracle; the reference draws them    */
/* from torch's Philox stream (nn.Dropout on the probabilities, MQ/libs/modeling/modeling_xlnet_x.py:308).                 */
int vilco_attn_dropout_mask(float* y, int64_t rows, int32_t cols, float p, uint32_t seed, void* stream);
/* Step word of the counter-based masks.  Every kernel that draws a dropout mask (vilco_dropout, vilco_act_bwd, the fused  */
/* epilogue dropout of vilco_gemm, the attention-probability dropout of vilco_attn_*) uses seed + word * 0x9E3779B1, where  */
/* `word` is ONE 32-bit value in device memory (0 after load: the effective seed is then the argument).  A training step    */
/* captured as a hipGraph replays its kernel arguments; with vilco_seed_word_bump as the graph's first node every replay    */
/* draws fresh masks, forward and backward of one replay the same ones.  (The reference draws from torch's Philox stream,  */
/* MQ/libs/modeling/blocks.py:226,268; modeling_xlnet_x.py:308: a stateful generator has no place in a replayed graph.)    */
/* _set / _bump are stream-ordered launches; _get synchronises the device (tests, logging).                                */
int vilco_seed_word_set(uint32_t value, void* stream);
int vilco_seed_word_bump(void* stream);
int vilco_seed_word_get(uint32_t* out);
/* out = alpha*a + beta*b (b may be null) */
int vilco_axpby(float* out, const float* a, const float* b, float alpha, float beta, int64_t n,
                void* stream);
/* dz = dropmask(dy) * act'(aux) * rowmask ; aux = pre-activation (gelu) or output (relu); act NONE = mask only */
typedef struct vilco_act_bwd_desc {
  const float* dy;       /* [rows][C] */
  const float* aux;
  float* dz;             /* may be NULL with planes (planes only) */
  float* dbias;          /* optional [C] = column sums of dz (needs workspace) */
  int32_t act;           /* VILCO_ACT_* */
  const int32_t* len;    /* optional prefix mask: row r -> b = r / T, t = r % T, zero when t >= len[b] */
  int32_t T;
  int64_t rows;
  int32_t C;
  /* drop_p > 0: the dropout mask (p, seed) of vilco_gemm's fused epilogue dropout, element index r*C + c */
  float drop_p;
  uint32_t drop_seed;
  void* workspace;       /* vilco_colsum_workspace(rows, C) bytes when dbias is wanted */
  size_t workspace_bytes;
  /* optional: partial maxima of |dz| (device, >= 2048 floats; *n_parts, HOST int32 = how many were written) */
  float* amax_parts;
  int32_t* n_parts;
  /* optional: dz written by this kernel as the fp16 x2 operand planes of its consumers -- no vilco_pack of dz follows.  `planes`:    */
  /* 256-byte aligned, vilco_act_bwd_planes_bytes() long.  seq_len = 0: vilco_pack's layout for [rows][C] at precision 3              */
  /* (C % 32 == 0).  seq_len > 0 (round 6): the k=3 convs' zero-padded per-sequence image (vilco_pack_item.seq_len: row (b, t) at      */
  /* b * (seq_len + 2) + 1 + t, the pad rows and the slack zeroed here; C % 8 == 0, rows % seq_len == 0) -- the output gradient of a   */
  /* masked k=3 conv (MQ/libs/modeling/blocks.py:79-84: conv output * mask) goes from the mask multiply straight into the operand      */
  /* image of its dX and weight-gradient products, no fp32 dz, no vilco_pack_many.  The planes' scale comes from a BOUND instead of    */
  /* the exact maximum: max|dy| (dy_amax: n_dy_amax partial maxima of |dy| left by the producer of dy, e.g.                            */
  /* vilco_gemm_desc.amax_out; required with planes) x 1 / (1 - drop_p) x max|act'|; it is the same power-of-two rule, at most two     */
  /* binary orders below the exact-maximum scale.                                                                                     */
  const float* dy_amax;
  int32_t n_dy_amax;
  void* planes;
  size_t planes_bytes;
  int32_t seq_len;
  const float* row_mask; /* as vilco_gemm_desc.row_mask (rows floats) or NULL */
} vilco_act_bwd_desc;
size_t vilco_act_bwd_planes_bytes(int64_t rows, int32_t C, int32_t seq_len);   /* size of `planes` for either layout */
int vilco_act_bwd(const vilco_act_bwd_desc* d, void* stream);
/* out[c] = sum_r x[r][c] */
int vilco_colsum(const float* x, float* out, int64_t rows, int32_t C, void* workspace,
                 size_t workspace_bytes, void* stream);
/* x[b][t][:] *= (t < len[b]) ; optional add: out = x + pe[t][c] * m  (backbones.py:222-226) */
int vilco_mask_rows(float* x, const int32_t* len, int32_t B, int32_t T, int32_t C, void* stream);
int vilco_add_pe(float* out, const float* x, const float* pe, const int32_t* len, int32_t B,
                 int32_t T, int32_t C, void* stream);
/* batched 2-D transpose: in[z][R][S] -> out[z][S][R]  (channel-first <-> token-major boundary) */
int vilco_transpose2d(const float* in, float* out, int32_t batch, int32_t R, int32_t S,
                      void* stream);
/* out[i][j][k] (contiguous, dims d0,d1,d2) = in[off + i*s0 + j*s1 + k*s2]  (conv weight permutes) */
int vilco_permute3(const float* in, float* out, int32_t d0, int32_t d1, int32_t d2, int64_t off,
                   int64_t s0, int64_t s1, int64_t s2, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* The chunk table every multi-tensor kernel walks (csrc/optim.hip), one block per chunk.                     */
/* A ROW is one stream of the operator: ptrs[k * n + t] is the address of tensor t's fp32 data in row k, so   */
/* entry t is the tuple (ptrs[0][t], ptrs[1][t], ...); each entry point names its rows and needs `rows` to be */
/* at least as many as it reads.  numel[t] = elements of entry t to walk, the same in every row: the whole    */
/* tensor, or a PREFIX of it when the class head has grown since the shorter row was made.  The work is cut   */
/* into nchunks chunks of at most `chunk` elements: chunk c covers elements chunk_off[c] .. of entry          */
/* chunk_tensor[c].  The chunks of one entry are consecutive and ascending, so per-chunk outputs (partial     */
/* sums, chunk_amax) of entry t are one contiguous run.  A chunk that lies outside its entry does nothing.    */
/* A null table, n < 0, nchunks < 0, chunk <= 0 or too few rows: VILCO_ERR_BADARG.                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_chunk_table {
  const int64_t* ptrs;         /* device [rows][n] */
  const int64_t* numel;        /* device [n] */
  const int32_t* chunk_tensor; /* device [nchunks] */
  const int64_t* chunk_off;    /* device [nchunks] */
  int32_t rows, n, nchunks, chunk;
} vilco_chunk_table;

/* ------------------------------------------------------------------------------------------ */
/* Step glue of train_one_epoch (MQ/libs/utils/train_utils.py:343-351): clip_grad_norm_ + optimizer.step()  */
/* as multi-tensor kernels over the n gradient-bearing fp32 tensors.                                         */
/* vilco_grad_norm reads row 1 (grad) of a table of >= 2 rows -- the optimizer's own table serves.           */
/* norm_coef (device float[2]) = {total L2 norm, min(1, max_norm/(norm+1e-6))};                              */
/* pass it to vilco_optim_step to scale gradients without a host sync, or null.                              */
/* kind 0 = torch.optim.AdamW (decoupled decay; tensor_step = device float[n], each tensor's step count      */
/* after this update, for the bias corrections), 1 = SGD with momentum.                                      */
/* lr / wd are HOST arrays indexed by parameter group (group[n] on the device).                              */
/* ------------------------------------------------------------------------------------------ */
int vilco_grad_norm(const vilco_chunk_table* table, float max_norm, float* partial, float* norm_coef, void* stream);
typedef struct vilco_optim_desc {
  vilco_chunk_table table;     /* rows: param, grad, exp_avg or momentum buffer, exp_avg_sq (AdamW reads 4, SGD 3) */
  int32_t kind;                /* 0 = AdamW, 1 = SGD with momentum */
  const int32_t* group;        /* device [n]: parameter group of every tensor */
  const float* lr;             /* HOST [ngroups] */
  const float* wd;             /* HOST [ngroups] */
  int32_t ngroups;             /* 1..8 */
  float beta1, beta2, eps, momentum;
  const float* tensor_step;    /* device [n] */
  const float* norm_coef;      /* vilco_grad_norm's, or NULL: gradients unscaled */
  /* optional: chunk_amax[c] (device float[nchunks]) = max|p| of the UPDATED parameter over chunk c: the chunks of one tensor are   */
  /* consecutive, so chunk_amax + first_chunk(t) with count chunks(t) is a vilco_pack_item.amax for next step's pack of weight t -- */
  /* the optimizer produces the scale of the fp16 x2 weight planes, the pack skips its own amax pass over the weight.               */
  float* chunk_amax;
  /* optional: the learning rates read from DEVICE memory (float[ngroups]; `lr` is then ignored): a training iteration captured as  */
  /* a hipGraph replays its arguments, so the per-iteration schedule value (MQ/libs/utils/lr_schedulers.py:71-104, stepped at       */
  /* train_utils.py:351) and the per-tensor step counts `tensor_step` are memory the host (or a captured increment) rewrites        */
  /* between replays.                                                                                                               */
  const float* lr_dev;
  /* optional (NULL: off): Synaptic Intelligence's path integral taken inside the update.  si_ptrs = device int64 [n]: the address of   */
  /* each tensor's omega (fp32, the parameter's element count, walked with the same chunk table), or 0 for a tensor that is not        */
  /* regularised.  Per element omega = fmaf(-gr, p_new - p_old, omega): gr = grad * clip coefficient (before SGD adds wd * p),          */
  /* p_new - p_old the fp32 difference of the stored values.  p and the optimizer state get the bits they get with NULL.  omega is     */
  /* memory a captured launch points at: it must outlive the graph, like the table.                                                    */
  const int64_t* si_ptrs;
} vilco_optim_desc;
int vilco_optim_step(const vilco_optim_desc* d, void* stream);
/* Synaptic Intelligence (Zenke et al. 2017), end of a task: ONE launch over all regularised tensors turns the path integral into  */
/* importance, in place:                                                                                                          */
/*   importance[i] = (i < numel_old[t] ? importance[i] : 0) + max(omega[i], 0) / ((p[i] - theta_start[i])^2 + xi)                   */
/*   optpar[i] = p[i];  omega[i] = 0;  theta_start[i] = p[i]                                   for i < numel[t]                    */
/* (quotient and sum in double, rounded once).  All five tensors of an entry hold numel[t] fp32 elements; importance beyond        */
/* numel_old[t] is not read (fresh memory; the new rows of a class head that has grown).  n <= 0, a null table, xi <= 0:           */
/* VILCO_ERR_BADARG.  nchunks == 0 launches nothing.                                                                              */
typedef struct vilco_si_desc {
  vilco_chunk_table table;     /* rows: param, omega, theta_start, importance, optpar; numel[t] = elements of the parameter */
  const int64_t* numel_old;    /* device [n]: leading elements of importance that held a value before, 0 .. numel[t] */
  float xi;                    /* > 0 (Zenke: 0.1) */
} vilco_si_desc;
int vilco_si_consolidate(const vilco_si_desc* d, void* stream);
/* RWalk (Riemannian Walk: Chaudhry, Dokania, Ajanthan, Torr, "Riemannian Walk for Incremental Learning: Understanding Forgetting   */
/* and Intransigence", ECCV 2018) inside the update: vilco_optim_step's update (p, the optimizer state and chunk_amax get the bits  */
/* they get there) which also keeps, per element of every tensor t with optim.si_ptrs[t] != 0, four fp32 states:                   */
/*   F  = fisher   <- F + alpha * (gr*gr - F)            gr as for si_ptrs; four roundings, in this order                           */
/*   w  = omega    <- fmaf(-gr, p_new - p_old, w)        optim.si_ptrs is its table                                                 */
/*   and when *tick % delta_t == 0 (a checkpoint update; *tick = iterations since the task began, counted after this one):          */
/*   s  = score    <- s + max(w, 0) / (0.5 * F * d*d + eps),  d = p_new - theta_ck   (new F and w; double, rounded once)            */
/*   w <- 0 ;  theta_ck <- p_new                                                                                                    */
/* score and theta_ck are neither read nor written by other updates; a tensor with si_ptrs[t] == 0 has none of its states touched.  */
/* tick is read from device memory by the kernel (a captured launch follows it); the caller advances it once per iteration.         */
/* EVERY block reads it, whether its tensor is tracked or not: it must be a device address whenever the call launches.             */
/* A NULL descriptor, NULL optim.si_ptrs / rw_ptrs / tick, alpha outside (0, 1], eps <= 0, delta_t < 1, and whatever                */
/* vilco_optim_step refuses: VILCO_ERR_BADARG before anything is read.                                                              */
typedef struct vilco_rwalk_step_desc {
  vilco_optim_desc optim;      /* si_ptrs = the omega table (required) */
  const int64_t* rw_ptrs;      /* device int64 [3][n]: fisher, score, theta_ck of tensor t (read only where si_ptrs[t] != 0) */
  const int32_t* tick;         /* device, one word */
  float alpha;                 /* in (0, 1]: the weight of the new squared gradient (the paper: 0.9) */
  float eps;                   /* > 0 */
  int32_t delta_t;             /* >= 1 (the paper: 10) */
} vilco_rwalk_step_desc;
int vilco_optim_step_rwalk(const vilco_rwalk_step_desc* d, void* stream);
/* RWalk, end of a task: three launches over all regularised tensors, no value read by the host.                                    */
/*   flush   s += max(w, 0) / (0.5 * F * (p - theta_ck)^2 + eps) (double, rounded once) ; w = 0 ; per-chunk max F and max s into     */
/*           partial (device float[2 * nchunks])                                                                                    */
/*   finish  out (device float[2]) = {max F, max s}; a NaN among them reaches out                                                   */
/*   apply   importance = F / maxF + s / maxS (double, rounded once; a term whose max is 0 contributes 0) ; optpar = p ;             */
/*           s = s / 2 ; theta_ck = p ; F is kept                                                                                   */
/* n <= 0, a null table / out_ptrs / partial / out, eps <= 0: VILCO_ERR_BADARG.  nchunks == 0 launches nothing.                     */
typedef struct vilco_rwalk_desc {
  vilco_chunk_table table;     /* rows: param, fisher, score, omega, theta_ck; numel[t] = elements of the parameter */
  const int64_t* out_ptrs;     /* device int64 [2][n]: importance, optpar (written, not read) */
  float* partial;              /* device float[2 * nchunks] */
  float* out;                  /* device float[2] */
  float eps;                   /* > 0 */
} vilco_rwalk_desc;
int vilco_rwalk_consolidate(const vilco_rwalk_desc* d, void* stream);
/* dst[0..n) = vals[0..n): n <= 16 HOST floats carried as kernel arguments (stream-ordered, no staging buffer) -- how the */
/* host hands this iteration's learning rates to a captured optimizer step.                                              */
int vilco_store_f32(float* dst, const float* vals, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* q/k/v pre-projection of MaskedMHCA fused with the block's first LayerNorm (MQ/libs/modeling/blocks.py:561-563 */
/* `self.ln1(x)`, :363-369 query/key/value_conv (depthwise k=3, stride 1|2, masked) + query/key/value_norm):       */
/*   h = LN1(x);  y_j = LN_j(dwconv3(h; w_j) * mask),  j = q, k, v.   One read of x, three writes (+ h on request).  */
/* w / gam / bet / y / mean / rstd are HOST arrays of three device pointers (q, k, v); w_j is the [C][1][3] conv    */
/* weight, gam_j / bet_j the [C] LayerNorm affine (the reference's [1,C,1] tensors).  mean1 / rstd1 [B*T] and       */
/* mean_j / rstd_j [B*T/stride] are kept for backward; h may be NULL.  C must be a multiple of 256, at most 2304.   */
/* Backward recomputes the conv outputs from h: dc_j (scratch, [B][T/stride][C] each) receives the gradient wrt the  */
/* masked conv outputs, dh = dh_ext (may be NULL) + the conv-transpose of the three; dparams (15 C floats) = d gam_q, */
/* d bet_q, d gam_k, d bet_k, d gam_v, d bet_v as [6][C], then d w_q, d w_k, d w_v as [3][C][3] (each the weight's    */
/* own [C][1][3] layout).  LN1's own backward is vilco_layernorm_bwd on (dh, x, mean1, rstd1).                       */
/* ------------------------------------------------------------------------------------------ */
int vilco_qkv_pre_supported(int32_t C);
/* amax_parts (may be NULL): three device arrays of vilco_qkv_pre_amax_parts(B, T, stride) floats that receive the        */
/* partial maxima of |q|, |k|, |v| (0 = too many partials: not emitted).                                                 */
int vilco_qkv_pre_amax_parts(int32_t B, int32_t T, int32_t stride);
int vilco_qkv_pre_fwd(const float* x, const float* ln1_g, const float* ln1_b, const float* const* w,
                      const float* const* gam, const float* const* bet, const int32_t* len, float* h,
                      float* const* y, float* mean1, float* rstd1, float* const* mean, float* const* rstd,
                      float* const* amax_parts, int32_t B, int32_t T, int32_t C, int32_t stride, float eps1, float eps,
                      void* stream);
size_t vilco_qkv_pre_bwd_workspace(int32_t B, int32_t T, int32_t C, int32_t stride);
int vilco_qkv_pre_bwd(const float* h, const float* const* w, const float* const* gam, const float* const* dy,
                      const float* const* mean, const float* const* rstd, const int32_t* len,
                      const float* dh_ext, float* const* dc, float* dh, float* dparams, int32_t B, int32_t T,
                      int32_t C, int32_t stride, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Point labelling + losses of the heads in two launches each way: label_points_single_video                    */
/* (MQ/libs/modeling/meta_archs.py:1253-1344), losses (:1374-1447: focal on valid points x gaussian weights,      */
/* DIoU on positives, "al" loss, loss_normalizer EMA :1407-1410), sigmoid_focal_loss / ctr_diou_loss_1d           */
/* (losses.py:5-52, 109-168) and the regression head's last two layers relu(Scale_l(x)) (meta_archs.py:344-346).   */
/* Rows r of a clip are the pyramid points of all levels laid end to end, optionally with separator rows           */
/* (points[r].stride <= 0).  gt = float [B][3*Nmax + 1]: Nmax (start, end) pairs, Nmax class ids, the count.        */
/* gauss = [6][C]: mu, sigma, mu_reg_left, sigma_reg_left, mu_reg_right, sigma_reg_right.                          */
/* loss_norm (device float[1]) is read and updated in place.  almax_state: device uint64 [B*C], zero before the    */
/* first call and left zero by every call.  out = {cls_loss, reg_loss, al_loss, cls + loss_weight*reg +            */
/* al_weight*al}; saved[0] = the normaliser used.  center_radius <= 0: center_sample 'none'.                       */
/* bwd: g_cls / g_reg / g_al / g_final = device scalars, the upstream gradients of the four outputs (NULL = 0).  */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_loss_desc {
  const float* logits;       /* [B][R][C] */
  const float* offsets;      /* [B][R][2] raw head output when level_scale != NULL, else already relu(scale * x) */
  const float* level_scale;  /* [L] or NULL */
  const float* points;       /* [R][4] = (t, reg_lo, reg_hi, stride) */
  const int32_t* row_level;  /* [R] */
  const int32_t* row_pos;    /* [R] position of the row inside its level */
  const int32_t* level_len;  /* [B][L] valid length of every level */
  const float* gt;           /* [B][3*Nmax + 1] */
  const float* gauss;        /* [6][C] */
  float* loss_norm;          /* [1] */
  int32_t B, R, C, L, Nmax;
  float center_radius, label_smoothing, momentum, loss_weight, al_weight;
  int32_t use_al;
} vilco_loss_desc;
size_t vilco_mq_loss_workspace(int32_t B, int32_t R, int32_t C);
int vilco_mq_loss_fwd(const vilco_loss_desc* d, float* out, float* saved, void* almax_state, void* workspace,
                      size_t workspace_bytes, void* stream);
/* backward: `workspace` is the forward's (its last region, B*R*8 floats, is scratch of THIS call: every row's share of the gradients of
 * the per-level regression scales and the gaussian-weight parameters, summed in a fixed order by a second launch -- no float atomics:
 * all gradients of a step are the same bits on every launch, round 6) */
int vilco_mq_loss_bwd(const vilco_loss_desc* d, const float* g_cls, const float* g_reg, const float* g_al,
                      const float* g_final, const float* saved, const void* workspace, float* d_logits,
                      float* d_offsets, float* d_level_scale, float* d_gauss, void* stream);
/* ER-ACE (Caccia et al., ICLR 2022): the same loss with a class window per clip.  cls_lo = DEVICE int32 [B], read when the
 * kernels run (a captured launch follows a table rewritten between replays); lo_b = cls_lo[b], a value outside [0, C) is
 * taken as 0.  For the rows of clip b the focal sum, the al softmax (a masked row: uniform 1/(C - lo_b)), the al maximum and
 * the al sum run over the columns [lo_b, C) only; targets, smoothing (C + 1), gaussian weights, the positive / negative
 * decision, the regression sum, #pos and the normaliser are those of the plain entries.  bwd writes d_logits[b, r, c] = 0 for
 * c < lo_b and assigns every element.  Workspace, almax_state, error returns (plus: cls_lo NULL -> VILCO_ERR_BADARG) and the
 * fixed summation order are the plain entries'; with cls_lo all zero every output is bit-identical to theirs. */
int vilco_mq_loss_ace_fwd(const vilco_loss_desc* d, const int32_t* cls_lo, float* out, float* saved, void* almax_state,
                          void* workspace, size_t workspace_bytes, void* stream);
int vilco_mq_loss_ace_bwd(const vilco_loss_desc* d, const int32_t* cls_lo, const float* g_cls, const float* g_reg,
                          const float* g_al, const float* g_final, const float* saved, const void* workspace,
                          float* d_logits, float* d_offsets, float* d_level_scale, float* d_gauss, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Distillation term of iCaRL / BiC (MQ/libs/modeling/meta_archs.py:1482-1519) and its gradient (csrc/distill.hip).  */
/* Per level l (rows level_row[l] .. + level_T[l] of batch row `clip`; padded positions count, as in the reference):  */
/*   mode 0 (iCaRL): out = 0.01 * sum_l (1/T_l) sum_t sum_{y < n_known} bce_with_logits(x[clip, t, y], p_l[t, y])       */
/*                   (`scale` is not read)                                                                              */
/*   mode 1 (BiC):   out = scale * sum_l -(1/T_l) sum_t sum_{y < n_known} p_l[t, y] log_softmax(x[clip, t, :n_known] / 2)[y] */
/* level_row / level_T are HOST arrays (validated before anything is enqueued); level_dev is their device copy,         */
/* int32 [2][L] (rows, then lengths), which the kernels walk -- rows it places outside the validated bounds are skipped.   */
/* fwd: two launches, fixed-order sums, out = device float[1].  bwd: one launch; g_out = device scalar, the upstream       */
/* gradient; ONLY d_logits[clip, level rows, :n_known] is written (assigned, not accumulated).  Same bits on every call.   */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_distill_desc {
  const float* logits;        /* [B][R][C] */
  const float* targets;       /* [sum T_l][ldt]: levels end to end, no separator rows */
  const int32_t* level_row;   /* host [L]: first row of every level inside R */
  const int32_t* level_T;     /* host [L]: rows of every level */
  const int32_t* level_dev;   /* device [2][L]: level_row, level_T */
  int32_t B, R, C, L;
  int32_t clip;               /* batch row the term reads (the reference: 0) */
  int32_t ldt;                /* row stride of targets, >= n_known */
  int32_t n_known;            /* 1 <= n_known <= min(C, ldt) */
  int32_t mode;               /* 0 iCaRL, 1 BiC */
  float scale;                /* BiC: 0.01 * n_known / n_classes */
} vilco_distill_desc;
size_t vilco_cl_distill_workspace(int64_t n_rows);      /* n_rows = sum T_l */
int vilco_cl_distill_fwd(const vilco_distill_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream);
int vilco_cl_distill_bwd(const vilco_distill_desc* d, const float* g_out, float* d_logits, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Dark Experience Replay (Buzzega et al., "Dark Experience for General Continual Learning", NeurIPS 2020; the reference   */
/* has no logit replay): every memory clip of the batch against the logits it produced when it entered the memory           */
/* (csrc/der.hip).  x = the concatenated head output [B][R][C] (level l in rows level_row[l] .. + level_T[l]); z_b = the    */
/* record of batch row b, fp32 [sum T_l][n_b], levels end to end without separators, n_b <= C (the head has grown since).   */
/*   der_tab   = DEVICE int64 [B][2]: der_tab[b][0] = address of z_b, or 0: row b has no record; der_tab[b][1] = n_b, the     */
/*               record's class count AND row stride.  A row with n_b outside [1, C] is skipped, not trusted.               */
/*   level_len = DEVICE int32 [B][L]: V_bl, the valid length of level l of row b (what vilco_loss_desc.level_len holds).     */
/*   S = sum_{b: rec} sum_l sum_{t < V_bl} sum_{y < n_b} (x[b, level_row[l] + t, y] - z_b[off_l + t, y])^2                  */
/*       (every term in fp32: one rounding for the difference, one for the square; the sum in fp64, in a fixed order)        */
/*   N = sum_{b: rec} n_b sum_l V_bl                                     (int64, formed on the device)                       */
/*   out  = (float)(alpha * S / N)   if N > 0, else 0                                                                        */
/*   c    = (float)(2.0 * alpha * g_out / N)                             (formed in double, rounded once)                    */
/*   d_logits[b, level_row[l] + t, y] = fl(fl(x - z) * c)   on exactly the compared elements                                */
/* level_row / level_T are HOST arrays (validated before anything is enqueued); level_dev is their device copy, int32      */
/* [2][L], which the kernels walk.  der_tab and level_len are read when the kernels RUN, so a captured launch follows a      */
/* table rewritten between replays; the records it names must stay where they are for as long as a graph may replay.        */
/* fwd: two launches; out = device float[1]; N is left in the workspace (vilco_der_workspace(B * sum T_l) bytes; the int64  */
/* at its first 256-byte boundary), where bwd reads it: hand bwd the SAME workspace, untouched in between.                   */
/* bwd: one launch; g_out = device scalar; the compared elements of d_logits are ASSIGNED and nothing else is written (the  */
/* caller supplies the zero-filled tensor); N == 0 writes nothing.  No atomics: the same bits on every call.                 */
/* A null pointer, L <= 0, B <= 0, a level outside R: VILCO_ERR_BADARG; a short workspace: VILCO_ERR_WORKSPACE -- both       */
/* before anything is enqueued.                                                                                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_der_desc {
  const float* logits;        /* [B][R][C] */
  const int32_t* level_row;   /* host [L]: first row of every level inside R */
  const int32_t* level_T;     /* host [L]: rows of every level */
  const int32_t* level_dev;   /* device [2][L]: level_row, level_T */
  const int32_t* level_len;   /* device [B][L]: valid lengths */
  const int64_t* der_tab;     /* device [B][2]: record address or 0, n_b */
  int32_t B, R, C, L;
  double alpha;               /* der_alpha */
} vilco_der_desc;
size_t vilco_der_workspace(int64_t n_pairs);            /* n_pairs = B * sum T_l */
int vilco_der_fwd(const vilco_der_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream);
int vilco_der_bwd(const vilco_der_desc* d, const float* g_out, float* d_logits, const void* workspace,
                  size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Pooled Outputs Distillation (Douillard et al., "PODNet", ECCV 2020; the reference has no feature-level distillation)   */
/* over the pyramid (csrc/pod.hip): h = feats[l][b], token-major [T_l][C]; V = level_len[b][l] clamped to [0, T_l].         */
/*   p[c] = sum_{t < V} fl(h[t][c]^2)   q[t] = sum_{c < C} fl(h[t][c]^2)   (squares fp32; sums fp64, fixed order)           */
/*   v = [p ; q] (C + V entries)   n = max(||v||, 1e-12)   u = fl32(v / n)  (fp64, rounded to fp32 once: what a record     */
/*   holds, so a clip against the record of its own features gives u - r = 0 and an exactly zero gradient)                 */
/*   r = the first C + V entries of the record's slice for level l; a record is fp32 [sum_l (C + T_l)], level l's slice     */
/*       [p (C) ; q (T_l)] at offset sum_{l' < l} (C + T_l'), stored normalised, any 4-byte alignment                      */
/*   dist[b][l] = ||u - r||  (0 for V == 0)   N_rec = rows with pod_tab[b] != 0, counted on the device                      */
/*   out = (float)(scale / (L N_rec) * sum_b sum_l dist[b][l]), 0 when N_rec == 0            (fp64, rounded once)           */
/*   g_u = w (u - r) / max(dist, 1e-12)   w = g_out scale / (L N_rec)   g_v = (g_u - u (u . g_u)) / n   (fp64, g_v rounded  */
/*   to fp32 once)   d_h[t][c] = fl(fl(2 h[t][c]) * fl(g_v[c] + g_v[C + t])) for t < V; 0 for t >= V and rows without record */
/* feats / level_T are HOST arrays (L <= 16 device pointers / lengths, validated before anything is enqueued).  pod_tab     */
/* (DEVICE int64 [B]: record address or 0) and level_len (DEVICE int32 [B][L]) are read when the kernels RUN, so a captured */
/* launch follows a table rewritten between replays; the records must stay where they are while a graph may replay.       */
/* fwd: three launches; out = device float[1]; N_rec is left in the workspace (the int64 at its first 256-byte boundary)   */
/* with g_v / w, where bwd reads them: hand bwd the SAME workspace, untouched in between.                                  */
/* bwd: one launch; g_out = device scalar; d_feats = host table of L device pointers; EVERY element of every level's        */
/* gradient is assigned (zeros where nothing is compared): the caller fills nothing.                                       */
/* record: two launches; every row is pooled (pod_tab is not read, may be null) and u is written to records [B][sum_l (C +  */
/* T_l)], entries t >= V as 0.  vilco_pod_tile_rows: the rows of a level one workgroup covers.  No atomics: same bits on    */
/* every call.  A null pointer, L outside 1..16, B < 1, C < 1, T_l < 1: VILCO_ERR_BADARG (vilco_pod_workspace: 0); a short  */
/* workspace: VILCO_ERR_WORKSPACE -- both before anything is enqueued.                                                     */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_pod_desc {
  const float* const* feats;  /* host [L]: device pointers, level l = [B][T_l][C] */
  const int32_t* level_T;     /* host [L]: rows of every level */
  const int32_t* level_len;   /* device [B][L]: valid lengths */
  const int64_t* pod_tab;     /* device [B]: record address or 0 */
  int32_t B, C, L, reserved;
  double scale;               /* pod_lambda * sqrt(n_classes / (n_classes - n_known)) */
} vilco_pod_desc;
int32_t vilco_pod_tile_rows(void);
size_t vilco_pod_workspace(const int32_t* level_T, int32_t L, int32_t B, int32_t C);
int vilco_pod_fwd(const vilco_pod_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream);
int vilco_pod_bwd(const vilco_pod_desc* d, const float* g_out, float* const* d_feats, const void* workspace,
                  size_t workspace_bytes, void* stream);
int vilco_pod_record(const vilco_pod_desc* d, float* records, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Elastic Response Distillation (Feng, Wang, Yuan, CVPR 2022; the reference has no method that holds the regression head)  */
/* (csrc/erd.hip; the definition is tests/erd_restatement.py).  Record time: z = the incoming model's logits [B][P][C],    */
/* levels end to end (P = sum T_l), o^ = its finished offsets [B][P][2]; V = the positions below level_len[b][l].          */
/*   c_i = max_{y < n_old} z_iy   mu = mean_V c   sigma = sqrt(mean_V (c - mu)^2)     (fp64, two passes, fixed order)       */
/*   S_cls = {i in V: c_i > mu + alpha_cls sigma}   S_reg = {i in V: c_i > mu + alpha_reg sigma and o^_i0 + o^_i1 > 0}      */
/* vilco_erd_select: two launches; conf [B][P] and flags [B][P] are scratch the fill reads again, counts [B][2] = |S_cls|,  */
/* |S_reg| per clip, which the HOST reads to size the buffers.  vilco_erd_select_fill: one launch; out_tab = DEVICE int64   */
/* [B][4] = the addresses of the clip's map_cls, map_reg (int32 [P]: position -> slot, ascending, -1 = not selected),      */
/* val_cls (fp32 [|S_cls|][n_old]) and val_reg (fp32 [|S_reg|][2]); slots come from a prefix scan, never from an atomic.    */
/* Every step: x = the concatenated head output [B][R][C], o = the offsets [B][R][2] in the same rows -- finished, or, with */
/* scale != null (DEVICE float [L], the fused loss route), raw: o = relu(fl32(scale_l raw)).                               */
/*   erd_tab = DEVICE int64 [B][5]: map_cls, map_reg, val_cls, val_reg, n_b (the record's class count and row stride), or   */
/*             zeros: row b has no record.  A row with n_b outside [1, C] is skipped, not trusted.                          */
/*   A = sum_b sum_{i in S_cls(b)} sum_{y < n_b} (x_iy - z_iy)^2   N_c = sum_b |S_cls(b)| n_b                               */
/*   D = sum_b sum_{i in S_reg(b)} diou(o_i, o^_i)                 N_r = sum_b |S_reg(b)|     (ctr_diou_loss_1d, eps 1e-8) */
/*   out[0..2] = lambda_cls A / N_c + lambda_reg D / N_r, its first part, its second part; a part whose count is 0 is 0.    */
/*   Terms fp64 from the fp32 inputs, sums fp64 in a fixed order, every output rounded to fp32 once.                        */
/* fwd: two launches; N_c, N_r (two int64 at the workspace's first 256-byte boundary) and the unweighted d scale are left   */
/* in the workspace (vilco_erd_workspace(B * sum T_l) bytes): hand bwd the SAME workspace, untouched in between.            */
/* bwd: one launch; g_out = device scalar; EVERY element of d_logits [B][R][C] and d_offsets [B][R][2] is assigned (zeros   */
/* where nothing is compared); with scale, d_offsets is the gradient of raw and d_scale [L] is written too.  The gradient   */
/* of diou takes autograd's choices: half to each side of a min / max tie, a clamp passes the gradient at >= eps.           */
/* erd_tab and level_len are read when the kernels RUN, so a captured launch follows a table rewritten between replays; the */
/* records must stay where they are while a graph may replay.  No atomics: the same bits on every call.  A null pointer,    */
/* L outside 1..16, B < 1, a level outside R, P != sum T_l, n_old outside 1..C: VILCO_ERR_BADARG; a short workspace:        */
/* VILCO_ERR_WORKSPACE -- both before anything is enqueued.                                                                */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_erd_desc {
  const float* logits;        /* [B][R][C] */
  const float* offsets;       /* [B][R][2] */
  const float* scale;         /* device [L], or null: offsets are finished */
  const int32_t* level_row;   /* host [L]: first row of every level inside R */
  const int32_t* level_T;     /* host [L]: rows of every level */
  const int32_t* level_dev;   /* device [2][L]: level_row, level_T */
  const int32_t* level_len;   /* device [B][L]: valid lengths */
  const int64_t* erd_tab;     /* device [B][5] */
  int32_t B, R, C, L;
  double lambda_cls, lambda_reg;
} vilco_erd_desc;
typedef struct vilco_erd_select_desc {
  const float* logits;        /* [B][P][C] */
  const float* offsets;       /* [B][P][2] */
  const int32_t* level_T;     /* host [L] */
  const int32_t* level_len;   /* device [B][L] */
  float* conf;                /* device [B][P] */
  int32_t* flags;             /* device [B][P] */
  int32_t* counts;            /* device [B][2] */
  const int64_t* out_tab;     /* device [B][4] (fill only) */
  int32_t B, P, C, n_old, L, reserved;
  double alpha_cls, alpha_reg;
} vilco_erd_select_desc;
int32_t vilco_erd_pairs_per_round(void);                /* (batch row, pyramid row) pairs one round of the forward grid covers */
size_t vilco_erd_workspace(int64_t n_pairs);            /* n_pairs = B * sum T_l */
int vilco_erd_fwd(const vilco_erd_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream);
int vilco_erd_bwd(const vilco_erd_desc* d, const float* g_out, float* d_logits, float* d_offsets, float* d_scale,
                  const void* workspace, size_t workspace_bytes, void* stream);
int vilco_erd_select(const vilco_erd_select_desc* d, void* stream);
int vilco_erd_select_fill(const vilco_erd_select_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* BiC bias correction of the classification head's output (MQ/libs/modeling/meta_archs.py:26-35: BiasLayer,           */
/* alpha * x + beta; :821-836: one layer per task over its slice of the class columns, the slices concatenated again)    */
/* as one launch over the concatenated head output (csrc/bic.hip):                                                       */
/*   y[r][c] = alpha[s(c)] * x[r][c] + beta[s(c)]   for every r < rows, c < C;   s(c) = i with splits[i-1] <= c < splits[i] */
/* The product and the sum are rounded separately (no FMA).  Every row gets the affine: separator rows of a level        */
/* layout and rows past a clip's valid length are not special.  Nothing outside [rows][C] is written.                    */
/* splits = HOST array of S cumulative ends, strictly increasing, splits[S-1] == C <= 128; it is validated before any     */
/* device work (empty, not increasing or not ending at C, n_layers != S: VILCO_ERR_BADARG; C > 128: _UNSUPPORTED).         */
/* table = DEVICE int64 [3][S]: the addresses of alpha_i (float[1]), the addresses of beta_i, the split ends again.     */
/* alpha and beta are read through it when the kernel runs -- never by the host -- so a captured launch sees the values  */
/* written after the capture.  A column the device table does not cover is not written.                                  */
/* fwd: one launch.  y may equal x (in place, ldy == ldx).                                                                */
/* bwd: the descriptor's x is the upstream gradient dy and y receives dx = alpha[s(c)] * dy (one launch; y may equal x).  */
/* dparams != NULL (some layer takes a gradient): device float [2][S] receives dalpha_i = sum dy * x_fwd and              */
/* dbeta_i = sum dy over all rows and the columns of split i -- two more launches, fixed-order fp64 sums without atomics,  */
/* the same bits on every call; x_fwd [rows][ld_fwd] is the forward's INPUT and `workspace` holds                         */
/* vilco_bic_correct_bwd_workspace(rows) bytes.  dparams == NULL: no reduction is launched, x_fwd / workspace are not read. */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_bic_correct_desc {
  const float* x;             /* [rows][ldx], the first C columns of every row */
  float* y;                   /* [rows][ldy] */
  const int32_t* splits;      /* host [S] */
  const int64_t* table;       /* device [3][S]: &alpha_i, &beta_i, splits[i] */
  int64_t rows;               /* B * R */
  int32_t C, S;
  int32_t ldx, ldy;           /* row strides in floats, >= C */
  int32_t n_layers;           /* layers the caller holds: must equal S */
} vilco_bic_correct_desc;
int vilco_bic_correct_fwd(const vilco_bic_correct_desc* d, void* stream);
size_t vilco_bic_correct_bwd_workspace(int64_t rows);
int vilco_bic_correct_bwd(const vilco_bic_correct_desc* d, const float* x_fwd, int32_t ld_fwd, float* dparams,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Continual-learning regularisers of MQ/libs/cl_methods/EWC.py:6-22 (get_regularized_loss) and MAS.py:5-21   */
/* (get_mas_regularized_loss), called per iteration from train_utils.py:337-344, as ONE multi-tensor launch:    */
/*   out[0] = lambda * sum_t sum_{i < numel[t]} F_t[i] (opt_t[i] - p_t[i])^2,   grad_t[i] -= 2 lambda F (opt - p) */
/* table rows (>= 4): parameter, its gradient (accumulated into), importance F (Fisher / |grad|), consolidated */
/* value opt; numel[t] = elements of opt_t (a prefix of the parameter when the class head has grown since the   */
/* task, EWC.py:19-21).  shared_params != 0: some parameter occurs in more than one entry (several consolidated */
/* tasks) -> gradient accumulated with atomics.                                                                 */
/* ------------------------------------------------------------------------------------------ */
int vilco_cl_penalty(const vilco_chunk_table* table, float lambda, int32_t shared_params, float* partial, float* out,
                     void* stream);
/* Importance accumulation of the consolidation passes MQ/libs/cl_methods/EWC.py:24-56 (on_task_update) and MAS.py:23-57        */
/* (on_task_mas_update), which keep the last batch's squared / absolute gradient; summing over the batches, and merging the   */
/* tasks (the commented-out consolidate_reg_params of MAS.py), is ONE multi-tensor launch over the same chunk table:           */
/*   acc_t[i] = beta * acc_t[i] + alpha * f(src_t[i])   for i < numel[t];   op 0: f(x) = x, 1: x * x, 2: |x|                  */
/* table rows (>= 2): src, acc.  numel[t] may be shorter than either allocation: elements past it are not touched.            */
/* beta == 0: acc is not read (fresh memory needs no memset, NaNs in it do not propagate); alpha == 0: src is not read.        */
/* Every element has one owner thread: no atomics, no workspace, the same bits on every call.  16-byte accesses wherever src  */
/* and acc are misaligned by the same amount, 4-byte accesses otherwise.  nchunks == 0 launches nothing.                       */
int vilco_cl_accumulate(const vilco_chunk_table* table, int32_t op, float alpha, float beta, void* stream);
/* A-GEM gradient projection (Chaudhry, Ranzato, Rohrbach, Elhoseiny: "Efficient Lifelong Learning with A-GEM", ICLR 2019,      */
/* eq. 11; the reference has no gradient-projection method, so there is no line of it to cite).  g = the step's gradient, r =   */
/* the gradient of a batch drawn from the replay memory, both taken over all entries of the table as ONE vector:               */
/*   g.r < 0 and r.r > 0:   g_t[i] <- fmaf(-alpha, r_t[i], g_t[i]),  alpha = (float)(g.r / r.r)        for i < numel[t]          */
/*   otherwise (no conflict, r = 0, a NaN dot):   alpha = 0 and g is neither read again nor written: it keeps its bits          */
/* table rows (>= 2): grad (fp32, projected in place), ref (fp32, read only); numel[t] = elements of both.                      */
/* partial = device float[2 * max(nchunks, 1)] (per-chunk fp32 sums of g r, then of r r: one read of the two streams, the       */
/* block reduction order of vilco_grad_norm); out = device float[3] = {g.r, r.r, alpha}, the two sums formed in double over     */
/* the partials and rounded once.  At most three launches (dot, finish, apply); the branch is taken on the device: no host      */
/* read, no allocation.  Every element has one owner thread: no atomics, the same bits on every call.  16-byte accesses where   */
/* grad and ref are misaligned by the same amount, 4-byte accesses otherwise.  nchunks == 0: out = {0, 0, 0}.                   */
/* A null table, rows < 2, a null partial or out: VILCO_ERR_BADARG, before anything is launched.                                */
int vilco_agem_project(const vilco_chunk_table* table, float* partial, float* out, void* stream);

/* Deferred finishing (csrc/defer.hip).  The second stage of every two-stage column reduction (LayerNorm d-gamma / d-beta,  */
/* bias and scale gradients, depthwise-tap gradients: reference autograd sums under blocks.py:152-166, 106-130, 628-641)  */
/* and the slab sum of a split-K product with a plain epilogue are small dependent launches whose results -- parameter     */
/* gradients -- nothing reads before backward ends.  While vilco_defer_set(1) is in force (process-wide) they are            */
/* recorded instead of launched; vilco_defer_flush(stream) issues all recorded items as a few batched launches (same       */
/* arithmetic, same order: bitwise the results of the individual launches) and switches recording off.  The partial buffers */
/* (workspaces) of recorded calls must stay alive until the flush.                                                        */
int vilco_defer_set(int32_t on);
int64_t vilco_defer_pending(void);
int vilco_defer_flush(void* stream);

/* ------------------------------------------------------------------------------------------ */
/* 1-D NMS on the device, replacing nms_1d_cpu (MQ/libs/utils/csrc/nms_cpu.cpp).                 */
/* Segments of all classes are passed concatenated; seg_off[nseg+1] gives each class's range      */
/* (batched_nms's per-class loop, nms.py:124-152, becomes one launch: one workgroup per class).   */
/* Outputs are per class at the same offsets: out_idx (indices LOCAL to the class, int64, in the  */
/* reference's return order) and out_cnt[nseg].  Index outputs are bit-exact vs the reference.    */
/* ------------------------------------------------------------------------------------------ */
size_t vilco_nms_workspace(int64_t n_total, int32_t nseg);
/* nms_cpu.cpp:19-58.  segs[n][2], scores[n]. */
int vilco_nms_1d(const float* segs, const float* scores, const int64_t* seg_off, int32_t nseg,
                 int64_t n_total, float iou_threshold, int64_t* out_idx, int64_t* out_cnt,
                 void* workspace, size_t workspace_bytes, void* stream);
/* nms_cpu.cpp:67-160.  dets[n][3] rows 0..cnt-1 of each class = (x1, x2, decayed score).
 * max_num > 0 stops each class after max_num picks (exact for the caller, nms.py:56-63). */
int vilco_softnms_1d(const float* segs, const float* scores, const int64_t* seg_off, int32_t nseg,
                     int64_t n_total, float iou_threshold, float sigma, float min_score,
                     int32_t method, int64_t max_num, float* dets, int64_t* out_idx,
                     int64_t* out_cnt, void* workspace, size_t workspace_bytes, void* stream);
/* Which device kernel a class of a vilco_softnms_1d call runs on is chosen per class from its size:
 *   kind 0  register-resident kernel (method 2 = Gaussian, nms_cpu.cpp:131-136; n <= 30 720)
 *   kind 1  row-strided kernel       (methods 0 / 1 / 2, nms_cpu.cpp:122-137;   n <= 65 536)
 *   kind 2  one-pass-per-pick kernel (any method, any n)
 * vilco_nms_set_kernel(-1) (the default) = the lowest kind that can take the class; kind k >= 0 = no kernel below kind k
 * (tests run every kernel on the same inputs this way).  Returns the previous setting.  All kernels produce the
 * reference's indices and scores bit for bit.  vilco_nms_last_kernels(): bit k set = the last vilco_softnms_1d call
 * launched kind k (host-side bookkeeping of the calling thread's last call; not synchronised). */
int vilco_nms_set_kernel(int32_t kind);
int vilco_nms_last_kernels(void);

/* ------------------------------------------------------------------------------------------ */
/* MQ evaluation on the device (evaluate.hip): ANETdetection's AP over tIoU thresholds           */
/* (MQ/libs/utils/metrics.py:274-393) and evaluation_retrieval's Recall@K                        */
/* (MQ/libs/utils/get_retrieval_performance.py:116-184).  All arithmetic fp64, match decisions    */
/* bit-identical; no float atomics (repeated calls are bitwise equal).  Threshold and rank lists   */
/* are HOST arrays (copied into kernel arguments); every other pointer is device memory.           */
/* ------------------------------------------------------------------------------------------ */
/* Detection AP.  pred_*[n_pred]: video index (outside [0, n_vid): no GT, every threshold an FP), */
/* class index (outside [0, n_cls): ignored), start, end, score.  Ground truth sorted into         */
/* (class, video) groups, each group's rows in the reference's GT order: gt_start / gt_end[n_gt],  */
/* grp_off[n_grp + 1] (grp_off[n_grp] == n_gt), grp_cls / grp_vid[n_grp]; cls_npos[n_cls] = GT     */
/* count per class.  Outputs ap[n_thr][n_cls] and, when tp_flags is not null, the TP flag of every */
/* prediction [n_thr][n_pred] in input order.  Score ties rank the later row first; tIoU ties      */
/* match the later GT first.  n_thr <= 16, n_cls < 65536, n_vid < 2^24 - 1 (else UNSUPPORTED).     */
/* A class with cls_npos == 0 has AP 0 whatever its predictions: the reference builds its class    */
/* index from the ground truth's labels, so it never scores such a class (no 0/0 recall here).     */
size_t vilco_det_ap_workspace(int64_t n_pred, int32_t n_gt, int32_t n_thr);
int vilco_det_ap(const int32_t* pred_vid, const int32_t* pred_cls, const double* pred_start, const double* pred_end,
                 const double* pred_score, int64_t n_pred, const double* gt_start, const double* gt_end,
                 const int32_t* grp_off, const int32_t* grp_cls, const int32_t* grp_vid, int32_t n_grp, int32_t n_gt,
                 const int32_t* cls_npos, int32_t n_cls, int32_t n_vid, const double* thresholds, int32_t n_thr,
                 double* ap, uint8_t* tp_flags, void* workspace, size_t workspace_bytes, void* stream);
/* Recall@K.  One group per (video, class name) of the ground truth: its GT rows                  */
/* gt_*[grp_gt_off[g] .. grp_gt_off[g + 1]) and its predictions, in result order,                 */
/* pred_*[grp_pred_off[g] .. + grp_pred_cnt[g]).  A GT is retrieved at (threshold t, rank r) when  */
/* one of the group's first r * n_gt predictions overlaps it by more than t (intersection over     */
/* the hull: iou(), get_retrieval_performance.py:166-184).  A NaN boundary on either side gives a  */
/* NaN overlap, which is no hit; so does the 0/0 of a zero-width hull.  A rank of 0 retrieves        */
/* nothing; a negative rank is BADARG.  Outputs hits[n_thr][n_rank] (int64 counts) and *total =     */
/* number of GT; recall = hits / total.  n_thr <= 16, n_rank <= 8.                                  */
size_t vilco_retrieval_hits_workspace(int32_t n_grp, int32_t n_thr, int32_t n_rank);
int vilco_retrieval_hits(const double* pred_start, const double* pred_end, const int32_t* grp_pred_off,
                         const int32_t* grp_pred_cnt, const double* gt_start, const double* gt_end,
                         const int32_t* grp_gt_off, int32_t n_grp, const double* thresholds, int32_t n_thr,
                         const int32_t* ranks, int32_t n_rank, int64_t* hits, int64_t* total, void* workspace,
                         size_t workspace_bytes, void* stream);
/* External classification scores fused into the detections (fuse.hip): the expansion of           */
/* postprocess_results (MQ/libs/utils/postprocessing.py:97-155).  Predictions are grouped by video:   */
/* pred_score / pred_start / pred_end[n_pred] (device, fp64), video v owns rows                       */
/* pred_off[v] .. pred_off[v + 1]; cls_score[n_vid][n_cls] (device, fp64) is the external class-score */
/* table.  Video v keeps its m = min(num_pred, rows) best rows by score and yields topk * m rows at    */
/* out_off[v]: the topk best classes by rank, inside a class the kept rows by rank; out_vid = v,       */
/* out_label = the class, out_start / out_end = the row's segment, out_score = sqrt(class score * row  */
/* score): one fp64 product and one correctly rounded square root, NaN for a negative product.  Both   */
/* rankings: descending value, equal values (and NaN, ranked first) with the larger index first.       */
/* pred_off and out_off[n_vid + 1] are HOST arrays; they are checked here (monotone from 0,            */
/* pred_off[n_vid] == n_pred, out_off[v + 1] - out_off[v] == topk * m, out_off[n_vid] == n_out) and     */
/* copied into the workspace with hipMemcpyAsync on the stream, so the call cannot be captured into a   */
/* graph.  1 <= topk <= n_cls and num_pred >= 1 (else BADARG), topk <= 64 (else UNSUPPORTED).  No       */
/* atomics: repeated calls are bitwise equal.                                                          */
size_t vilco_score_fuse_workspace(int64_t n_pred, int32_t n_vid);
int vilco_score_fuse(const double* pred_score, const double* pred_start, const double* pred_end,
                     const int32_t* pred_off, int64_t n_pred, int32_t n_vid, const double* cls_score, int32_t n_cls,
                     int32_t num_pred, int32_t topk, const int32_t* out_off, int64_t n_out, int32_t* out_vid,
                     int32_t* out_label, double* out_start, double* out_end, double* out_score, void* workspace,
                     size_t workspace_bytes, void* stream);
/* NLQ Recall@K over IoU and mIoU (ReferringRecall).  Query q has one ground-truth window           */
/* gt[q] = (start, end), fp64, and pred_cnt[q] predictions pred[q][0 .. cnt) = (start, end) in        */
/* result order, 0 <= cnt <= k_cap; rows past the count are never read.  pred is fp32 when            */
/* pred_fp32 != 0, else fp64; gt must be 16-byte aligned, pred 8 (fp32) or 16 (fp64).  seg_id[q] in   */
/* [0, n_seg) is the segment (template, task) of the query; null: one segment; ids outside the        */
/* range are counted nowhere.  mode 0: fp64, intersection and hull clamped at 0 (NumPy               */
/* compute_IoU); mode 1: operands rounded to fp32, intersection clamped, hull not, correctly          */
/* rounded fp32 quotient widened to fp64 (torch _iou).  A 0/0 IoU is NaN and NaN is not > t.          */
/* Outputs: hits[n_seg][n_thr][n_rank] = queries of the segment for which one of the first            */
/* min(ranks[r], cnt) predictions has IoU > thresholds[t]; n[n_seg] = queries per segment;            */
/* top1[n_query] = IoU of the first prediction (NaN when cnt == 0); top1_sum[n_seg] = its sum per     */
/* segment in a fixed order (repeated calls are bit-equal); flags (optional)                          */
/* [n_query][n_thr][n_rank].  n_thr <= 16, n_rank <= 8 (else UNSUPPORTED), ranks >= 1, k_cap >= 1.    */
size_t vilco_nlq_recall_workspace(int64_t n_query, int32_t n_rank);
int vilco_nlq_recall(const void* pred, int32_t pred_fp32, const int32_t* pred_cnt, int32_t k_cap, const double* gt,
                     const int32_t* seg_id, int64_t n_query, int32_t n_seg, const double* thresholds, int32_t n_thr,
                     const int32_t* ranks, int32_t n_rank, int32_t mode, int64_t* hits, int64_t* n, double* top1,
                     double* top1_sum, uint8_t* flags, void* workspace, size_t workspace_bytes, void* stream);
/* NLQ model ensembling (ensemble.hip): the per-query recipe of NLQ/ensemble.py:7-101, 123-143 with  */
/* NLQ/temporal_nms.py:6-74, all queries in one launch.  pred[n_model][n_query][k_cap][3] holds rows  */
/* (start, end, score) in result order, fp32 when pred_fp32 != 0, else fp64; cnt[n_model][n_query]    */
/* the rows present (clamped to [0, k_cap]; rows past the count are never read).  Per query:          */
/* the first top1_max_input rows of every model, in model order, go through top1_generator: keyed by  */
/* centre (end + start) / 2, of equal centres the last row stays; centres ascending; a centre joins   */
/* the cluster while centre - previous centre < distance; per cluster total = the scores summed left   */
/* to right, "max" = the first row of maximal score, "middle" = row (c - 1) / 2 for an odd count c,    */
/* for an even one row c / 2 if its score is greater than that of row c / 2 - 1, else that row; the    */
/* proposal is (middle + max) / 2 in start, end and score; proposals by total descending, ties in      */
/* centre order.  The fusion list = the first max_input rows of model 0, 1, ..., then the proposals    */
/* (scored by their averaged score).  NMS: stable order by score descending; greedily keep the head   */
/* and drop every later row with overlap > nms_thd, overlap = max(0, min(e) - max(s)) / (max(e) -      */
/* min(s)), 0 when that span is 0; at most max_after_nms rows.  out[n_query][max_after_nms][3] (fp64)  */
/* = the kept rows (start, end, score); rows past the kept ones repeat the last one when pad != 0,     */
/* else are 0; out_cnt[n_query] = rows kept before padding.  Optional (both or neither):               */
/* prop[n_query][n_model * top1_max_input][4] = the proposals (start, end, score, total) in their      */
/* order, rows past prop_cnt[n_query] untouched.  top1_max_input = 0 switches the generator off: with  */
/* n_model = 1 the call is a batched temporal_nms.  All arithmetic is fp64 in the reference's order:   */
/* bit-equal to CPython for finite inputs (NaN has no defined order there).  Limits (else BADARG, as   */
/* for null pointers with n_query > 0): 1 <= n_model <= 8, 1 <= max_input <= 10, k_cap >=              */
/* max_input, n_model * top1_max_input <= 64, n_model * (max_input + min(top1_max_input, k_cap)) <=    */
/* 128, 1 <= max_after_nms <= 128.  No workspace, no atomics, no host synchronisation.                 */
int vilco_nlq_ensemble(const void* pred, int32_t pred_fp32, const int32_t* cnt, int32_t n_model, int64_t n_query,
                       int32_t k_cap, int32_t max_input, int32_t top1_max_input, double distance, double nms_thd,
                       int32_t max_after_nms, int32_t pad, double* out, int32_t* out_cnt, double* prop,
                       int32_t* prop_cnt, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Herding exemplar selection for the replay memory (herding.hip).  Replaces the reference's      */
/* commented-out, unfinished branch MQ/libs/modeling/meta_archs.py:973-1043 (two pdb.set_trace(),  */
/* a norm over the wrong axis, features[idx] indexed across levels); the random sampling that      */
/* runs instead is :1046-1052.  A clip's descriptor is its feature pyramid, phi[i][l] = level-l    */
/* map / its Frobenius norm (what `classify`, :1061-1131, averages).  With G[l] = Phi[l] Phi[l]^T: */
/*   mu[l] = mean_i phi[i][l] / its norm,   a_i = mu . phi_i = rowsum_i(G) / sqrt(sum(G)),          */
/*   mu . (phi_i + S) = a_i + sum_{j in sel} a_j,                                                  */
/*   ||phi_i + S||^2 = G_ii + 2 sum_{j in sel} G_ij + sum_{j,j' in sel} G_jj',                      */
/*   cost(i) = sum_l ( 2 - 2 (mu . (phi_i + S)) / ||phi_i + S|| ).                                 */
/* No allocation, no host synchronisation, no float atomics; repeated calls are bit-equal.         */
/* ------------------------------------------------------------------------------------------ */
/* inv_norm[r] = 1 / ||x[r, 0:D]||_2 for the rows of fp32 x[rows][ld] (rows <= 65535, ld >= D):    */
/* fp32 squares, per-thread fp32 sums, fixed trees and the sum over segments in fp64.              */
size_t vilco_frob_scale_workspace(int64_t rows, int64_t D);
int vilco_frob_scale(const float* x, int64_t rows, int64_t D, int64_t ld, float* inv_norm, void* workspace,
                     size_t workspace_bytes, void* stream);
/* G[N][N] = diag(row_scale) X X^T diag(row_scale) for fp32 X[N][ld] (row_scale null: ones).       */
/* Exact fp32 products and fp32 accumulation (v_mfma_f32_32x32x2_f32) inside each of the K slabs   */
/* the chip is split over, the slabs' partials added in slab order in fp64; G is written as fp32   */
/* (g_fp64 == 0) or fp64 and is exactly symmetric.  Row offsets are 64-bit: N * D is not limited   */
/* to 2^31 bytes as a vilco_gemm operand is.  N <= 32767.  The workspace holds the partials.       */
size_t vilco_gram_workspace(int64_t N, int64_t D);
int vilco_gram(const float* x, int64_t N, int64_t D, int64_t ld, const float* row_scale, void* g, int32_t g_fp64,
               void* workspace, size_t workspace_bytes, void* stream);
/* Greedy herding order.  grams: fp64 [n_cls][L][N][N] (every class N candidates, L levels),        */
/* sel: int32 [n_cls][min(m, N)].  One workgroup per class, all arithmetic fp64 without            */
/* contraction in the order written above: rowsum_i = sum_j G[i][j] in index order, sum(G) = the    */
/* row sums in index order, cost = the levels in order; after a pick p: s += 2 r_p + G_pp,          */
/* t += a_p, r_i += G[p][i].  Smallest cost wins, ties (and NaN, ranked as +inf) go to the smallest */
/* index.  L <= 16, N <= 4096 (else UNSUPPORTED).                                                  */
size_t vilco_herd_select_workspace(int32_t n_cls, int32_t L, int32_t N);
int vilco_herd_select(const double* grams, int32_t n_cls, int32_t L, int32_t N, int32_t m, int32_t* sel,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* BiC stage 2 (bic.hip): fit (alpha, beta) of the newest BiasLayer on held-out clips with the     */
/* network frozen.  Replaces the reference's second phase, MQ/train_bic.py:602-649 with            */
/* train_bic_one_epoch's per-step model forward, PtTransformer.losses                              */
/* (MQ/libs/modeling/meta_archs.py:1374-1447, the focal term) and backward to the two scalars --   */
/* whose optimizer (train_bic.py:622) the reference never steps.  The cache (built once, the       */
/* network is frozen) holds all points of all held-out clips, clip after clip:                     */
/*   logits[N][C] fp32 raw classification logits (before the bias correction), C <= 128;           */
/*   label_bits[N][2] uint64, bit c = (gt_cls[n][c] == 1);  weight[N] fp32 = valid * w_cls (w_cls  */
/*   is 1 on negatives; 0 on padded points);  pos[N] uint8 = pos_mask;  clip_ptr[n_clips + 1]      */
/*   int32 row offsets (empty clips allowed).  For a set S of clips and the columns [lo, hi):      */
/*   L = (1 / max(P, 1)) sum_{n in S} weight[n] sum_{c in [lo,hi)} focal(alpha x[n][c] + beta, t), */
/*   P = sum_{n in S} pos[n],  t = bit (1 - smoothing) + smoothing / (C + 1),  focal =             */
/*   sigmoid_focal_loss with alpha 0.25, gamma 2 (losses.py:5-52).                                 */
/* Per-element arithmetic is fp32; the sums are fp64 from the thread upward in a fixed order: two  */
/* calls give bit-equal results.  No atomics, no grid barrier, no host synchronisation.            */
/* BADARG: C > 128, lo >= hi, hi > C, batch_clips <= 0, null pointers.  N < 2^24.                  */
/* ------------------------------------------------------------------------------------------ */
/* n_steps plain-SGD steps, step k over the clips order[k * batch_clips .. (k + 1) * batch_clips)  */
/* (device int32; indices outside [0, n_clips) are skipped).  ab_inout[2] = (alpha, beta) fp32 on  */
/* the device, read once and rewritten after every step; the trajectory itself is kept in fp64.    */
/* loss_out[n_steps] fp64 = L of every step before its update.  Two launches per step, ordered by  */
/* the stream.                                                                                     */
size_t vilco_bic_fit_ws_bytes(int64_t N, int32_t n_clips, int32_t batch_clips, int32_t lo, int32_t hi);
int vilco_bic_fit(const float* logits, const uint64_t* label_bits, const float* weight, const uint8_t* pos,
                  const int32_t* clip_ptr, int64_t N, int32_t n_clips, const int32_t* order, int32_t n_steps,
                  int32_t batch_clips, int32_t C, int32_t lo, int32_t hi, float smoothing, double lr, float* ab_inout,
                  double* loss_out, void* ws, size_t ws_size, void* stream);
/* One pass over all clips: out3 = (L, dL/dalpha, dL/dbeta) fp64 at ab[2] = (alpha, beta) fp32.    */
size_t vilco_bic_eval_ws_bytes(int64_t N, int32_t n_clips, int32_t lo, int32_t hi);
int vilco_bic_eval(const float* logits, const uint64_t* label_bits, const float* weight, const uint8_t* pos,
                   const int32_t* clip_ptr, int64_t N, int32_t n_clips, int32_t C, int32_t lo, int32_t hi, float smoothing,
                   const float* ab, double* out3, void* ws, size_t ws_size, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Narration SSL of the ViLCo recipe (ssl.hip).  Replaces, in MQ/libs/modeling/meta_archs.py,      */
/* the masked mean poolings of forward (:794-811), MemoryBank.update (:38-60), the branch          */
/* :939-945 and masked_contrastive_loss (:1351-1372) -- without their host reads (the mask sum,    */
/* the boolean indexing, the Python ring pointer), so the step can be captured and replayed.       */
/* fp32, wave64, fixed-order two-stage sums, no atomics: repeated calls are bit-equal.             */
/* ------------------------------------------------------------------------------------------ */
/* out[B][C] = (1/L) sum_l (1/max(len[b][l], 1)) sum_{t < len[b][l]} feats[l][b][t][:].            */
/* feats: HOST array of L device pointers to token-major fp32 [B][T[l]][C]; T: host int32[L];      */
/* lens: device int32 [B][L] prefix lengths (clamped to [0, T[l]]; 0 contributes zero, as the      */
/* reference's denom[denom == 0] = 1).  Elements at or above the length are never read.  L = 1     */
/* pools the narration encoder's output over the token lengths.  BADARG: L < 1, L > 16, B < 1,     */
/* C < 1, T[l] < 1, null pointers.  The workspace holds the per-slab partials.                     */
size_t vilco_ssl_pool_workspace(const int32_t* T, int32_t L, int32_t B, int32_t C);
int vilco_ssl_pool_fwd(const float* const* feats, const int32_t* T, int32_t L, const int32_t* lens, int32_t B,
                       int32_t C, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* dfeats[l][b][t][:] = dout[b][:] / (L max(len, 1)) for t < len, 0 for len <= t < T[l].            */
int vilco_ssl_pool_bwd(const float* dout, float* const* dfeats, const int32_t* T, int32_t L, const int32_t* lens,
                       int32_t B, int32_t C, void* stream);
/* InfoNCE against the memory bank.  text, video: raw pooled rows [B][D]; mask: float [B], a row   */
/* takes part when mask[b] != 0; bank [M][D]; ring: device int32[1], the bank's write position.    */
/* In the reference's order: (1) both inputs are L2-normalised (x / max(||x||, 1e-12)) into        */
/* xn[2][B][D]; (2) the masked normalised text rows, compacted in batch order, are written to      */
/* bank rows (ring + rank) mod M and ring advances by their count n modulo M -- a launch of its    */
/* own, so the loss sees the rows just written among its negatives; (3) per masked row and         */
/* modality, logits [pos, x . bank_j ...] / temperature and their log-sum-exp;                     */
/*   loss[0] = sum_masked ((lse_t - pos/temp) + (lse_v - pos/temp)) / (2 n).                       */
/* n == 0: loss = 0, bank and ring untouched.  Saved for the backward: xn, stats[7 B] = (norms     */
/* [2][B], pos [B], lse as shift [2][B] + log of the shifted sum [2][B]), logits [2 B][M] in fp64   */
/* (accumulated in fp64: at temperature 0.07 fp32 rounding of a logit is 4e-6 of its probability). */
/* BADARG: D % 4 != 0, D > 4096, B < 1, B > 64, B > M (the reference's assert), temperature <= 0,  */
/* null or misaligned pointers.                                                                    */
size_t vilco_ssl_nce_workspace(int32_t B, int32_t D, int32_t M);
int vilco_ssl_nce_fwd(const float* text, const float* video, const float* mask, int32_t B, int32_t D, float* bank,
                      int32_t M, int32_t* ring, float temperature, float* xn, float* stats, double* logits,
                      float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* dtext, dvideo [B][D]: gradients of gloss[0] * loss with respect to the RAW text and video rows  */
/* (through the normalisation, the positive pair's cross term in both); the bank must be what the  */
/* forward left.  Unmasked rows and n == 0 give exact zeros.  The bank gets no gradient.           */
int vilco_ssl_nce_bwd(const float* gloss, const float* mask, const float* xn, const float* stats, const double* logits,
                      const float* bank, int32_t B, int32_t D, int32_t M, float temperature, float* dtext,
                      float* dvideo, void* workspace, size_t workspace_bytes, void* stream);
/* Step (2) alone, for rows that are normalised already (MemoryBank.update_masked).                */
int vilco_ssl_ring_update(const float* rows, const float* mask, int32_t B, int32_t D, float* bank, int32_t M,
                          int32_t* ring, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* L2P prompt pool (MQ/libs/cl_methods/prompt.py:47-117): match, batch vote and prepend (csrc/prompt.hip).          */
/*   row key   xk[b] = mean_l x[b][l] | max_l | max + 2 mean | cls[b]   (key_mode; padding rows count)                 */
/*   normalise xn[b] = xk[b] rsqrt(max(sum xk^2, 1e-12)), pn[p] likewise from key[p];  sim[b][p] = <xn[b], pn[p]>      */
/*   select    idx_in given: idx = idx_in (entries outside [0, P) raise the status word and are clamped).             */
/*             idx_in NULL: per row the k prompts of largest sim by COUNTING RANK (before = larger sim, or equal sim   */
/*             and smaller index; NaN is out of contract); vote != 0: the k ids with the most picks over all B k       */
/*             picks, again by counting rank (larger count, equal counts by smaller id), the same list for every row.  */
/*   outputs   prompted[b] = prompt[idx[b][0]], ..., prompt[idx[b][k-1]] (len rows each), then x[b]  -- bit copies;    */
/*             reduce_sim = (sum_b (sum_j sim[b][idx[b][j]])) / B, j then b in order;  selkey[b][j] = pn[idx[b][j]].    */
/* fwd: two launches (select: one workgroup per row; gather-and-prepend: row copies, idx read from device memory).    */
/* bwd: at most two launches.  g_prompted [B][k len + L][C], g_reduce_sim device float[1].  d_prompt[p] = the sum of  */
/* g_prompted[b][j len .. (j+1) len) over the (b, j) with idx[b][j] == p in (b, j) order (exact zeros when none);      */
/* d_key through reduce_sim and the normalisation; d_x = g_prompted[:, k len:] + the reduce_sim path through the row   */
/* key (max: to the FIRST position attaining it; key_mode 3 has none).  Each of d_prompt / d_key / d_x may be NULL.    */
/* No float atomics: the same bits on every call.  `workspace` (vilco_prompt_workspace bytes, 256-byte aligned) is     */
/* written by fwd and read by bwd: keep it between the two.                                                            */
/* BADARG before any device work: !(1 <= k <= P <= 64), len < 1, B < 1, L < 1, C < 1, key_mode outside 0..3, key_mode  */
/* 3 without cls, null operands.                                                                                       */
/* ------------------------------------------------------------------------------------------ */
enum { VILCO_PROMPT_MEAN = 0, VILCO_PROMPT_MAX = 1, VILCO_PROMPT_MEAN_MAX = 2, VILCO_PROMPT_CLS = 3 };
typedef struct vilco_prompt_desc {
  const float* x;           /* [B][L][C] */
  const float* prompt;      /* [P][len][C] */
  const float* key;         /* [P][C] */
  const float* cls;         /* [B][C], key_mode 3 only */
  const int64_t* idx_in;    /* [B][k] or NULL: select on the device */
  int32_t B, L, C, P, len, k;
  int32_t key_mode;         /* VILCO_PROMPT_* */
  int32_t vote;             /* batchwise_prompt; only read when idx_in is NULL */
  /* outputs of fwd (inputs of bwd: idx, xn, pn) */
  int64_t* idx;             /* [B][k] */
  float* sim;               /* [B][P] */
  float* pn;                /* [P][C] */
  float* xn;                /* [B][C] */
  float* selkey;            /* [B][k][C] */
  float* prompted;          /* [B][k len + L][C] */
  float* reduce_sim;        /* [1] */
  void* workspace;
  size_t workspace_bytes;
} vilco_prompt_desc;
size_t vilco_prompt_workspace(const vilco_prompt_desc* d);
int vilco_prompt_fwd(const vilco_prompt_desc* d, void* stream);
int vilco_prompt_bwd(const vilco_prompt_desc* d, const float* g_prompted, const float* g_reduce_sim, float* d_prompt,
                     float* d_key, float* d_x, void* stream);
/* The library's device status word: kernels that validate device-resident arguments (vilco_prompt_fwd: idx_in) OR a    */
/* bit into it instead of faulting or making the host read.  _take synchronises the device, returns the word and clears */
/* it (tests, end-of-epoch checks); bit 0 = a prompt index outside [0, P).                                               */
int vilco_status_word_take(int32_t* out);

/* ------------------------------------------------------------------------------------------ */
/* CODA-Prompt (Smith et al., "CODA-Prompt: COntinual Decomposed Attention-based Prompting for Rehearsal-Free         */
/* Continual Learning", CVPR 2023): soft weighting of the pool's components, prepend (csrc/coda.hip).  The reference   */
/* project has no counterpart; tests/coda_restatement.py states the same formulas in float64.                          */
/*   query     xk[b] = mean_l x[b][l] over all L rows (padding rows count, as in the L2P op's mean mode)                */
/*   weights   for m < f: u = xk[b] (.) attn[m];  alpha[b][m] = <u, key[m]> / (max(|u|, 1e-12) max(|key[m]|, 1e-12))    */
/*             (F.normalize semantics: a zero vector gives exactly 0);  alpha[b][m] = 0 for m >= f                      */
/*   outputs   prompted[b] = [ sum_{m < f} alpha[b][m] prompt[m] (in order of m) ; x[b] ]  -- the x rows are bit copies;  */
/*             want_ortho: ortho = pen(key[:f]) + pen(attn[:f]) + pen(prompt[:f] as [f][len C]),                        */
/*             pen(T) = mean over the f x f entries of (T T^t - I)^2;  otherwise no Gram launch and ortho = 0 exactly.  */
/* fwd: two launches, three with want_ortho.  bwd: at most two.  g_prompted [B][len + L][C], g_ortho device float[1]    */
/* (read with want_ortho only).  The query is a constant (d_x = g_prompted[:, len:] is the caller's view, no launch);   */
/* g_alpha[b][m] = <g_prompted[b][:len], prompt[m]>;  d_prompt[m] = sum_b alpha[b][m] g_prompted[b][:len];  d_key and    */
/* d_attn through the cosine: d alpha / d u = (k^ - alpha u^) / |u|, d alpha / d key = (u^ - alpha k^) / |key|,          */
/* d_attn[m] = sum_b g_alpha xk[b] (.) d alpha / d u, a norm below the clamp treated as the clamp's constant; plus the   */
/* penalty's g_ortho 4 / f^2 (T T^t - I) T.  Sums over b in order.  Rows [s, f) only: rows [0, s) (frozen, detached in   */
/* the method) and [f, M) (unused) of all three gradients are exact zeros.  Each of d_prompt / d_key / d_attn may be    */
/* NULL.  alpha is handed out in fp32 and kept in fp64 in the workspace: every other value is computed from the fp64    */
/* copy.  No host read, no float atomics, fp64 sums in a fixed order: the same bits on every call.  `workspace`         */
/* (vilco_coda_workspace bytes, 256-byte aligned) is written by fwd and read by bwd: keep it between the two.           */
/* BADARG before any device work: !(1 <= f <= M <= 128), !(0 <= s < f), len, B, L, C < 1, null operands.                */
/* ------------------------------------------------------------------------------------------ */
typedef struct vilco_coda_desc {
  const float* x;           /* [B][L][C] */
  const float* prompt;      /* [M][len][C] */
  const float* key;         /* [M][C] */
  const float* attn;        /* [M][C] */
  int32_t B, L, C, M, len;
  int32_t s, f;             /* the task's rows [s, f); rows [0, s) are used but frozen, rows [f, M) unused */
  int32_t want_ortho;
  /* outputs of fwd */
  float* alpha;             /* [B][M] */
  float* prompted;          /* [B][len + L][C] */
  float* ortho;             /* [1] */
  void* workspace;
  size_t workspace_bytes;
} vilco_coda_desc;
size_t vilco_coda_workspace(const vilco_coda_desc* d);
int vilco_coda_fwd(const vilco_coda_desc* d, void* stream);
int vilco_coda_bwd(const vilco_coda_desc* d, const float* g_prompted, const float* g_ortho, float* d_prompt,
                   float* d_key, float* d_attn, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VILCO_HIP_H */
