// L2P prompt pool (MQ/libs/cl_methods/prompt.py:47-117): query key, cosine match against the pool's keys, per-row top-k,
// batch vote, gather-and-prepend, the pull term reduce_sim -- and the gradients of prompt, key and x.  The problem is
// latency-bound (B <= 32 rows, P <= 64 prompts, C = 512 / 768, L <= ~100 tokens, <= ~1 MB copied): what is spent is
// launches and dependent round trips, so the forward is two launches and the backward at most two, whatever B, k and P.
//
//   prompt_select_kernel   one workgroup of 8 waves per batch row b.  (1) row key: lanes own channel groups (float4 when C % 4
//                          == 0), the waves split L into slices; a slice's sum / first maximum is formed in row order, the
//                          slices are combined in slice order through LDS.  (2) sum xk^2 over lanes, then waves, in order;
//                          xn = xk rsqrt(max(., 1e-12)).  (3) one wave per prompt p: sum key^2, pn = key rsqrt(.), sim =
//                          <xn, pn> (row 0's workgroup also writes pn).  (4) thread p: counting rank of sim[b][p] -- the number of
//                          prompts that come first (larger sim, or equal sim and smaller index), as ensemble.hip orders its
//                          rows -- and the k first go to the row's list.  All of it in fp64, rounded once where a value is
//                          written out (ranks are taken before that rounding; equal inputs give equal bits either way).  A given idx is range-checked here instead: a bad
//                          entry ORs bit 0 into the library's status word and is clamped, nothing is read out of bounds.
//   prompt_gather_kernel   every workgroup reads the B k row picks into LDS and, with the vote on, recounts them (thread p counts
//                          id p; counting rank again: larger count, equal counts by smaller id): B k <= 2048 LDS reads are
//                          cheaper than a launch or a grid-wide handshake.  Then one wave per output row: prompt rows, text
//                          rows and the selected keys are bit copies (float4, scalar rows when C % 4 != 0).  Workgroup 0 also
//                          writes idx and reduce_sim = (sum_b (sum_j sim[b][idx[b][j]])) / B, j then b in order.
//                          The reference pads torch.unique's result to P entries with count 0 before its second topk
//                          (prompt.py:76-78).  Every row contributes k DISTINCT ids, so at least k ids have a count >= 1 and a
//                          padding entry (count 0) can never be among the k largest: it needs no counterpart here.
//   prompt_bwd_key_kernel  workgroups 0 .. B-1: d xk[b] (workspace) = J_norm (g / B) sum_j pn[idx[b][j]];  workgroups B .. B+P-1:
//                          d key[p] = J_norm (g / B) sum_{(b,j): idx = p} xn[b] in (b, j) order.  J_norm y = rs (y - n <n, y>), or
//                          rs y where the eps clamp was active.
//   prompt_bwd_row_kernel  one wave per row: d x[b][l] = g_prompted[b][k len + l] + d xk[b] / L (mean) + d xk[b] where l is the
//                          first position of the maximum; d prompt[p][t] = sum of g_prompted[b][j len + t] over the picks of p in
//                          (b, j) order, exact zeros without a pick.  Every output element has one owner: no atomics.
#include "common.h"

namespace {

constexpr int ST = 512;                // select: threads per workgroup (8 waves; its LDS partials are fp64)
constexpr int SW = ST / 64;
constexpr int RT = 256;                // row kernels: threads per workgroup (4 waves, one row each)
constexpr int RW = RT / 64;
constexpr int MAX_P = 64;
constexpr int MAX_PICKS = 2048;        // B k, held in LDS by every workgroup of the row kernels
constexpr int MAX_GRID = 2048;
constexpr double NORM_EPS = 1e-12;

struct PromptArgs {
  const float* x; const float* prompt; const float* key; const float* cls; const int64_t* idx_in;
  int64_t* idx; float* sim; float* pn; float* xn; float* selkey; float* prompted; float* reduce_sim;
  double* ssq;                         // workspace: [B] sum xk^2 of the row keys, then [P] of the pool keys
  double* simd;                        // workspace: [B][P] the similarities before their rounding to fp32
  int32_t* rowidx;                     // workspace: [B][k] the row's picks (or the given, clamped window)
  int32_t* arg;                        // workspace: [B][C] first position of the maximum
  double* dscr;                        // workspace: [B][C] forward: the row key xk; backward: its gradient
  int32_t* status;
  int B, L, C, P, len, k, key_mode, vote;
  int vec;                             // 4: float4 rows (C % 4 == 0, 16-byte aligned operands), 1: scalar rows
  int gw, S;                           // select: waves that span the channel groups, slices of L
};

struct Layout { size_t ssq, simd, rowidx, arg, dscr, total; };

Layout layout(long B, long C, long P, long k) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  Layout l;
  l.ssq = 0;
  l.simd = up((size_t)(B + P) * 8);
  l.rowidx = l.simd + up((size_t)(B * P) * 8);
  l.arg = l.rowidx + up((size_t)(B * k) * 4);
  l.dscr = l.arg + up((size_t)(B * C) * 4);
  l.total = l.dscr + up((size_t)(B * C) * 8);
  return l;
}

// The small reductions (row key, norms, dot products, reduce_sim, the gradient sums) run in fp64 and are rounded to fp32
// once, where a value leaves the kernel: B, P, C and L are tiny against the machine, the cost is launches and round
// trips, not flops -- and the results sit at the rounding of their fp32 inputs and outputs instead of a summation order's.
// sum over the wavefront in a fixed butterfly order, in every lane (all 64 lanes active)
__device__ __forceinline__ double wave_sum_d(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

// sum over the workgroup in a fixed order (lanes, then waves 0, 1, ...), in every thread; NW waves, all threads call it
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  v = wave_sum_d(v);
  __syncthreads();                     // s_red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_red[0];
  for (int w = 1; w < NW; ++w) t = t + s_red[w];
  return t;
}

__global__ __launch_bounds__(ST) void prompt_select_kernel(PromptArgs a) {
  __shared__ double s_sum[ST * 4];
  __shared__ float s_max[ST * 4];
  __shared__ int s_arg[ST * 4];
  __shared__ double s_red[SW];
  __shared__ double s_sim[MAX_P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, C = a.C, L = a.L;
  float* xn = a.xn + (long)b * C;
  double* xk = a.dscr + (long)b * C;

  // ---- (1) the row key xk[b] (workspace, fp64)
  if (a.key_mode != VILCO_PROMPT_CLS) {
    const int vec = a.vec, G = C / vec, tile = a.gw * 64;
    const int s = wave / a.gw, gl = (wave % a.gw) * 64 + lane;
    const int l0 = (int)((long)s * L / a.S), l1 = (int)((long)(s + 1) * L / a.S);      // S <= L: no slice is empty
    const float* xb = a.x + (long)b * L * C;
    for (int g0 = 0; g0 < G; g0 += tile) {                                              // workgroup-uniform
      const int g = g0 + gl;
      const bool mine = s < a.S && g < G;
      double sum[4] = {0.0, 0.0, 0.0, 0.0};
      float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      int ar[4] = {l0, l0, l0, l0};
      if (mine) {
        if (vec == 4) {
          for (int l = l0; l < l1; ++l) {
            const float4 v = *reinterpret_cast<const float4*>(xb + (long)l * C + g * 4);
            const float e[4] = {v.x, v.y, v.z, v.w};
            for (int i = 0; i < 4; ++i) {
              sum[i] = sum[i] + (double)e[i];
              if (e[i] > mx[i]) { mx[i] = e[i]; ar[i] = l; }                            // strict: the first maximum stays
            }
          }
        } else {
          for (int l = l0; l < l1; ++l) {
            const float e = xb[(long)l * C + g];
            sum[0] = sum[0] + (double)e;
            if (e > mx[0]) { mx[0] = e; ar[0] = l; }
          }
        }
        const int o = (s * tile + gl) * 4;                                              // (s, gl) < (S, tile), S gw <= SW
        for (int i = 0; i < vec; ++i) { s_sum[o + i] = sum[i]; s_max[o + i] = mx[i]; s_arg[o + i] = ar[i]; }
      }
      __syncthreads();
      if (mine && s == 0) {
        for (int i = 0; i < vec; ++i) {
          double t = sum[i];
          float m = mx[i];
          int at = ar[i];
          for (int q = 1; q < a.S; ++q) {                                               // slices in order
            const int o = (q * tile + gl) * 4 + i;
            t = t + s_sum[o];
            if (s_max[o] > m) { m = s_max[o]; at = s_arg[o]; }
          }
          const double mean = t / (double)L;
          const int c = g * vec + i;
          xk[c] = a.key_mode == VILCO_PROMPT_MEAN ? mean : (a.key_mode == VILCO_PROMPT_MAX ? (double)m : (double)m + 2.0 * mean);
          a.arg[(long)b * C + c] = at;
        }
      }
      __syncthreads();
    }
  }

  // ---- (2) normalise
  if (a.key_mode == VILCO_PROMPT_CLS)
    for (int c = tid; c < C; c += ST) xk[c] = (double)a.cls[(long)b * C + c];           // read back below by the thread that wrote it
  double q = 0.0;
  for (int c = tid; c < C; c += ST) q = q + xk[c] * xk[c];
  const double ssq = block_sum<SW>(q, s_red);                                           // (its barriers also publish xk)
  const double rs = 1.0 / sqrt(fmax(ssq, NORM_EPS));
  if (tid == 0) a.ssq[b] = ssq;
  for (int c = tid; c < C; c += ST) xn[c] = (float)(xk[c] * rs);

  // ---- (3) one wave per prompt
  for (int p = wave; p < a.P; p += SW) {                                                // wave-uniform
    const float* kr = a.key + (long)p * C;
    double kq = 0.0;
    for (int c = lane; c < C; c += 64) kq = kq + (double)kr[c] * (double)kr[c];
    kq = wave_sum_d(kq);
    const double rk = 1.0 / sqrt(fmax(kq, NORM_EPS));
    double d = 0.0;
    for (int c = lane; c < C; c += 64) {
      d = d + xk[c] * (double)kr[c];
      if (b == 0) a.pn[(long)p * C + c] = (float)((double)kr[c] * rk);
    }
    d = wave_sum_d(d) * rs * rk;                                                        // <xn, pn> before xn and pn are rounded
    if (lane == 0) {
      a.sim[(long)b * a.P + p] = (float)d;
      a.simd[(long)b * a.P + p] = d;
      s_sim[p] = d;
      if (b == 0) a.ssq[a.B + p] = kq;
    }
  }
  __syncthreads();

  // ---- (4) the row's list
  if (a.idx_in == nullptr) {
    if (tid < a.P) {
      const double v = s_sim[tid];
      int r = 0;
      for (int j = 0; j < a.P; ++j) {
        const double y = s_sim[j];
        r += (y > v || (y == v && j < tid)) ? 1 : 0;
      }
      if (r < a.k) a.rowidx[b * a.k + r] = tid;
    }
  } else if (tid < a.k) {
    long v = a.idx_in[(long)b * a.k + tid];
    if (v < 0 || v >= a.P) {
      atomicOr(a.status, 1);
      v = v < 0 ? 0 : a.P - 1;
    }
    a.rowidx[b * a.k + tid] = (int)v;
  }
}

// the B k picks in LDS; with the vote on, replaced by the voted list for every row
__device__ __forceinline__ void load_picks(const PromptArgs& a, int* s_idx, int* s_cnt, int* s_final) {
  const int tid = threadIdx.x, n = a.B * a.k;
  for (int i = tid; i < n; i += RT) s_idx[i] = a.rowidx[i];
  __syncthreads();
  if (a.vote && a.idx_in == nullptr) {                                                  // workgroup-uniform
    if (tid < MAX_P) {
      int c = -1;
      if (tid < a.P) {
        c = 0;
        for (int i = 0; i < n; ++i) c += s_idx[i] == tid ? 1 : 0;
      }
      s_cnt[tid] = c;
    }
    __syncthreads();
    if (tid < a.P) {
      const int v = s_cnt[tid];
      int r = 0;
      for (int j = 0; j < a.P; ++j) {
        const int y = s_cnt[j];
        r += (y > v || (y == v && j < tid)) ? 1 : 0;
      }
      if (r < a.k) s_final[r] = tid;
    }
    __syncthreads();
    for (int i = tid; i < n; i += RT) s_idx[i] = s_final[i % a.k];
    __syncthreads();
  }
}

__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int C, int vec, int lane) {
  if (vec == 4) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int c = lane; c < C / 4; c += 64) d4[c] = s4[c];
  } else {
    for (int c = lane; c < C; c += 64) dst[c] = src[c];
  }
}

__global__ __launch_bounds__(RT) void prompt_gather_kernel(PromptArgs a) {
  __shared__ int s_idx[MAX_PICKS];
  __shared__ int s_cnt[MAX_P];
  __shared__ int s_final[MAX_P];
  __shared__ double s_row[RT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = a.B * a.k;
  load_picks(a, s_idx, s_cnt, s_final);
  if (blockIdx.x == 0) {
    for (int i = tid; i < n; i += RT) a.idx[i] = (int64_t)s_idx[i];
    if (tid < a.B) {
      double r = 0.0;
      for (int j = 0; j < a.k; ++j) r = r + a.simd[(long)tid * a.P + s_idx[tid * a.k + j]];
      s_row[tid] = r;
    }
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int b = 0; b < a.B; ++b) t = t + s_row[b];
      a.reduce_sim[0] = (float)(t / (double)a.B);
    }
  }
  const long T = (long)a.k * a.len + a.L, main_rows = (long)a.B * T, rows = main_rows + n;
  for (long r = (long)blockIdx.x * RW + wave; r < rows; r += (long)gridDim.x * RW) {     // wave-uniform
    const float* src;
    float* dst;
    if (r < main_rows) {
      const long b = r / T, t = r - b * T;
      if (t < (long)a.k * a.len) {
        const int j = (int)(t / a.len), u = (int)(t - (long)j * a.len);
        src = a.prompt + ((long)s_idx[b * a.k + j] * a.len + u) * a.C;
      } else {
        src = a.x + (b * a.L + (t - (long)a.k * a.len)) * a.C;
      }
      dst = a.prompted + r * a.C;
    } else {
      const long i = r - main_rows;
      src = a.pn + (long)s_idx[i] * a.C;
      dst = a.selkey + i * a.C;
    }
    copy_row(src, dst, a.C, a.vec, lane);
  }
}

// the picks as the forward left them in idx (clamped again: the tensor is the caller's by now)
__device__ __forceinline__ void load_idx(const PromptArgs& a, int* s_idx) {
  const int n = a.B * a.k;
  for (int i = threadIdx.x; i < n; i += RT) {
    const long v = a.idx[i];
    s_idx[i] = v < 0 ? 0 : (v >= a.P ? a.P - 1 : (int)v);
  }
  __syncthreads();
}

__global__ __launch_bounds__(RT) void prompt_bwd_key_kernel(PromptArgs a, const float* __restrict__ g_rs, float* __restrict__ d_key,
                                                            int want_x) {
  __shared__ int s_idx[MAX_PICKS];
  __shared__ double s_red[RW];
  const int tid = threadIdx.x, C = a.C, n = a.B * a.k;
  const bool row = (int)blockIdx.x < a.B;
  if (row ? !want_x : d_key == nullptr) return;                                         // workgroup-uniform
  load_idx(a, s_idx);
  const double g = (double)g_rs[0] / (double)a.B;
  if (row) {
    const int b = blockIdx.x;
    const float* xn = a.xn + (long)b * C;
    double dot = 0.0;
    for (int c = tid; c < C; c += RT) {
      double u = 0.0;
      for (int j = 0; j < a.k; ++j) u = u + (double)a.pn[(long)s_idx[b * a.k + j] * C + c];
      dot = dot + (double)xn[c] * (g * u);
    }
    dot = block_sum<RW>(dot, s_red);
    const double ssq = a.ssq[b], rs = 1.0 / sqrt(fmax(ssq, NORM_EPS));
    const bool free_norm = ssq >= NORM_EPS;                                             // clamp_min passes the gradient at equality
    for (int c = tid; c < C; c += RT) {
      double u = 0.0;
      for (int j = 0; j < a.k; ++j) u = u + (double)a.pn[(long)s_idx[b * a.k + j] * C + c];
      const double y = g * u;
      a.dscr[(long)b * C + c] = free_norm ? rs * (y - (double)xn[c] * dot) : rs * y;
    }
  } else {
    const int p = blockIdx.x - a.B;
    const float* pn = a.pn + (long)p * C;
    double dot = 0.0;
    for (int c = tid; c < C; c += RT) {
      double v = 0.0;
      for (int i = 0; i < n; ++i)
        if (s_idx[i] == p) v = v + (double)a.xn[(long)(i / a.k) * C + c];
      dot = dot + (double)pn[c] * (g * v);
    }
    dot = block_sum<RW>(dot, s_red);
    const double ssq = a.ssq[a.B + p], rs = 1.0 / sqrt(fmax(ssq, NORM_EPS));
    const bool free_norm = ssq >= NORM_EPS;
    for (int c = tid; c < C; c += RT) {
      double v = 0.0;
      for (int i = 0; i < n; ++i)
        if (s_idx[i] == p) v = v + (double)a.xn[(long)(i / a.k) * C + c];
      const double y = g * v;
      d_key[(long)p * C + c] = (float)(free_norm ? rs * (y - (double)pn[c] * dot) : rs * y);
    }
  }
}

__global__ __launch_bounds__(RT) void prompt_bwd_row_kernel(PromptArgs a, const float* __restrict__ gp, float* __restrict__ d_prompt,
                                                            float* __restrict__ d_x, int path, int vec) {
  __shared__ int s_idx[MAX_PICKS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, n = a.B * a.k;
  load_idx(a, s_idx);
  const long T = (long)a.k * a.len + a.L;
  const long x_rows = d_x ? (long)a.B * a.L : 0, p_rows = d_prompt ? (long)a.P * a.len : 0;
  // d xk reaches x[b][l] as mean_w / L (the mean) and, at the first position of the maximum, once more
  const double mean_w = (a.key_mode == VILCO_PROMPT_MEAN ? 1.0 : (a.key_mode == VILCO_PROMPT_MEAN_MAX ? 2.0 : 0.0)) / (double)a.L;
  const bool has_max = a.key_mode == VILCO_PROMPT_MAX || a.key_mode == VILCO_PROMPT_MEAN_MAX;
  const int step = vec * 64;
  for (long r = (long)blockIdx.x * RW + wave; r < x_rows + p_rows; r += (long)gridDim.x * RW) {      // wave-uniform
    if (r < x_rows) {
      const long b = r / a.L;
      const int l = (int)(r - b * a.L);
      const float* src = gp + (b * T + (long)a.k * a.len + l) * C;
      const double* dk = a.dscr + b * C;
      const int* ag = a.arg + b * C;
      float* dst = d_x + r * C;
      for (int c = lane * vec; c < C; c += step) {
        float e[4];
        if (vec == 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + c);
          e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        } else {
          e[0] = src[c];
        }
        if (path)
          for (int i = 0; i < vec; ++i) {
            const double d = dk[c + i];
            double v = (double)e[i] + mean_w * d;
            if (has_max && ag[c + i] == l) v = v + d;
            e[i] = (float)v;
          }
        if (vec == 4) *reinterpret_cast<float4*>(dst + c) = make_float4(e[0], e[1], e[2], e[3]);
        else dst[c] = e[0];
      }
    } else {
      const long q = r - x_rows;
      const int p = (int)(q / a.len), t = (int)(q - (long)p * a.len);
      float* dst = d_prompt + q * C;
      for (int c = lane * vec; c < C; c += step) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < n; ++i)                                                       // (b, j) order
          if (s_idx[i] == p) {
            const int b = i / a.k, j = i - b * a.k;
            const float* g = gp + ((long)b * T + (long)j * a.len + t) * C + c;
            if (vec == 4) {
              const float4 v = *reinterpret_cast<const float4*>(g);
              acc[0] = acc[0] + (double)v.x; acc[1] = acc[1] + (double)v.y;
              acc[2] = acc[2] + (double)v.z; acc[3] = acc[3] + (double)v.w;
            } else {
              acc[0] = acc[0] + (double)g[0];
            }
          }
        if (vec == 4) *reinterpret_cast<float4*>(dst + c) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
        else dst[c] = (float)acc[0];
      }
    }
  }
}

// everything a launch relies on, checked on the host before any device work
int check_desc(const vilco_prompt_desc* d) {
  if (!d) return VILCO_ERR_BADARG;
  if (d->B < 1 || d->L < 1 || d->C < 1 || d->len < 1) return VILCO_ERR_BADARG;
  if (d->k < 1 || d->k > d->P || d->P > MAX_P) return VILCO_ERR_BADARG;
  if (d->key_mode < VILCO_PROMPT_MEAN || d->key_mode > VILCO_PROMPT_CLS) return VILCO_ERR_BADARG;
  if (d->key_mode == VILCO_PROMPT_CLS && !d->cls) return VILCO_ERR_BADARG;
  if ((long)d->B * d->k > MAX_PICKS || d->B > RT) return VILCO_ERR_UNSUPPORTED;      // the picks live in LDS, one thread per row sums
  if (!d->x || !d->prompt || !d->key || !d->idx || !d->sim || !d->pn || !d->xn || !d->selkey || !d->prompted || !d->reduce_sim)
    return VILCO_ERR_BADARG;
  if (!d->workspace || !vilco_aligned(d->workspace, 256)) return VILCO_ERR_BADARG;
  if (d->workspace_bytes < layout(d->B, d->C, d->P, d->k).total) return VILCO_ERR_WORKSPACE;
  return VILCO_OK;
}

PromptArgs make_args(const vilco_prompt_desc* d) {
  PromptArgs a;
  a.x = d->x; a.prompt = d->prompt; a.key = d->key; a.cls = d->cls; a.idx_in = d->idx_in;
  a.idx = d->idx; a.sim = d->sim; a.pn = d->pn; a.xn = d->xn; a.selkey = d->selkey; a.prompted = d->prompted;
  a.reduce_sim = d->reduce_sim;
  const Layout l = layout(d->B, d->C, d->P, d->k);
  unsigned char* w = reinterpret_cast<unsigned char*>(d->workspace);
  a.ssq = reinterpret_cast<double*>(w + l.ssq);
  a.simd = reinterpret_cast<double*>(w + l.simd);
  a.rowidx = reinterpret_cast<int32_t*>(w + l.rowidx);
  a.arg = reinterpret_cast<int32_t*>(w + l.arg);
  a.dscr = reinterpret_cast<double*>(w + l.dscr);
  a.status = nullptr;
  a.B = d->B; a.L = d->L; a.C = d->C; a.P = d->P; a.len = d->len; a.k = d->k; a.key_mode = d->key_mode;
  a.vote = d->vote != 0 && d->idx_in == nullptr;
  a.vec = (d->C % 4 == 0 && vilco_aligned(d->x, 16) && vilco_aligned(d->prompt, 16) && vilco_aligned(d->pn, 16) &&
           vilco_aligned(d->selkey, 16) && vilco_aligned(d->prompted, 16)) ? 4 : 1;
  const int G = d->C / a.vec, gwfull = (G + 63) / 64;
  a.gw = gwfull < SW ? gwfull : SW;
  a.S = SW / a.gw < d->L ? SW / a.gw : d->L;
  return a;
}

int row_grid(long rows) {
  const long g = (rows + RW - 1) / RW;
  return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

}  // namespace

extern "C" size_t vilco_prompt_workspace(const vilco_prompt_desc* d) {
  if (!d || d->B < 1 || d->C < 1 || d->P < 1 || d->k < 1) return 0;
  return layout(d->B, d->C, d->P, d->k).total;
}

extern "C" int vilco_prompt_fwd(const vilco_prompt_desc* d, void* stream) {
  const int rc = check_desc(d);
  if (rc != VILCO_OK) return rc;
  PromptArgs a = make_args(d);
  a.status = vilco_status_word_dev();
  if (!a.status) return VILCO_ERR_LAUNCH;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(prompt_select_kernel, dim3(d->B), dim3(ST), 0, s, a);
  const long rows = (long)d->B * ((long)d->k * d->len + d->L) + (long)d->B * d->k;
  hipLaunchKernelGGL(prompt_gather_kernel, dim3(row_grid(rows)), dim3(RT), 0, s, a);
  return vilco_launch_status();
}

extern "C" int vilco_prompt_bwd(const vilco_prompt_desc* d, const float* g_prompted, const float* g_reduce_sim, float* d_prompt,
                                float* d_key, float* d_x, void* stream) {
  const int rc = check_desc(d);
  if (rc != VILCO_OK) return rc;
  if (!g_prompted || !g_reduce_sim) return VILCO_ERR_BADARG;
  if (!d_prompt && !d_key && !d_x) return VILCO_OK;
  const PromptArgs a = make_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int path = d_x != nullptr && d->key_mode != VILCO_PROMPT_CLS;                    // reduce_sim reaches x through the row key
  if (path || d_key)
    hipLaunchKernelGGL(prompt_bwd_key_kernel, dim3(d->B + d->P), dim3(RT), 0, s, a, g_reduce_sim, d_key, path);
  if (d_x || d_prompt) {
    const int vec = (d->C % 4 == 0 && vilco_aligned(g_prompted, 16) && (!d_x || vilco_aligned(d_x, 16)) &&
                     (!d_prompt || vilco_aligned(d_prompt, 16))) ? 4 : 1;
    const long rows = (d_x ? (long)d->B * d->L : 0) + (d_prompt ? (long)d->P * d->len : 0);
    hipLaunchKernelGGL(prompt_bwd_row_kernel, dim3(row_grid(rows)), dim3(RT), 0, s, a, g_prompted, d_prompt, d_x, path, vec);
  }
  return vilco_launch_status();
}
