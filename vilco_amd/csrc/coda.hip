// CODA-Prompt (Smith et al., "CODA-Prompt: COntinual Decomposed Attention-based Prompting for Rehearsal-Free Continual
// Learning", CVPR 2023): the soft, fully differentiable successor of the L2P pool in prompt.hip.  The formulas are the ones
// include/vilco_hip.h states for vilco_coda_desc.  Like the L2P op the problem is latency-bound (B <= 32 rows, M <= 128
// components, C = 768, L <= ~100 tokens): what is spent is launches, so the forward is two launches (three with the
// orthogonality penalty) and the backward at most two, whatever B, M and f.
//
//   coda_alpha_kernel     one workgroup of 8 waves per batch row b.  (1) xk[b] = mean_l x[b][l]: lanes own channel groups
//                         (float4 when C % 4 == 0), the waves split L into slices, a slice is summed in row order and the
//                         slices are combined in slice order through LDS; xk stays fp64 in the workspace.  (2) one wave per
//                         component m < f: u = xk (.) A[m], the three sums <u, u>, <K, K>, <u, K> over lanes in a fixed
//                         butterfly order, alpha = <u, K> / (max(|u|, eps) max(|K|, eps)).  alpha is written twice: rounded
//                         to fp32 for the caller, and fp64 into the workspace together with |u|^2 and |K|^2 -- every later
//                         kernel reads the fp64 copy, so no value passes through an fp32 alpha.  Columns m >= f: zeros.
//   coda_gram_kernel      (want_ortho only) one wave per entry (i <= j) of the three f x f Gram matrices of K[:f], A[:f] and
//                         prompt[:f] viewed as [f, len C]: G = T T^t - I goes to the workspace (both triangles; the backward
//                         multiplies by it), the workgroup's sum of G^2 to a partial.
//   coda_mix_kernel       one wave per output row: p[b][t] = sum_{m < f} alpha[b][m] prompt[m][t] in order of m, fp64, rounded
//                         once; text rows are bit copies (float4, scalar rows when C % 4 != 0).  Workgroup 0 adds the Gram
//                         partials in order and writes ortho = sum / f^2 (an exact 0 without want_ortho).
//   coda_bwd_dot_kernel   one wave per (b, m in [s, f)): g_alpha[b][m] = <g_prompted[b][:len], prompt[m]> (workspace, fp64).
//   coda_bwd_rows_kernel  one wave per row of d_prompt, and one per component for d_key and d_attn together: sums over b in
//                         order, the penalty's 4 g_ortho / f^2 (G T)[m] added from the workspace's Gram, rows outside [s, f)
//                         written as exact zeros.  Every output element has one owner: no atomics.
#include "common.h"

namespace {

constexpr int ST = 512;                // alpha: threads per workgroup (8 waves)
constexpr int SW = ST / 64;
constexpr int RT = 256;                // row kernels: threads per workgroup (4 waves, one row each)
constexpr int RW = RT / 64;
constexpr int MAX_M = 128;
constexpr int MAX_GRID = 2048;
constexpr double NORM_EPS = 1e-12;

struct CodaArgs {
  const float* x; const float* prompt; const float* key; const float* attn;
  float* alpha; float* prompted; float* ortho;
  double* xk;                          // workspace: [B][C] the query, mean over the L rows
  double* alphad;                      // workspace: [B][M] alpha before its rounding to fp32 (columns < f)
  double* uu;                          // workspace: [B][M] |xk[b] (.) A[m]|^2
  double* kk;                          // workspace: [M] |K[m]|^2
  double* ga;                          // workspace: [B][M] backward: d loss / d alpha (columns [s, f))
  double* gram;                        // workspace: [3][f][f] T T^t - I of key, attn, prompt
  double* parts;                       // workspace: [MAX_GRID] the Gram workgroups' sums of squares
  int B, L, C, M, len, s, f, want_ortho;
  int vec;                             // 4: float4 rows (C % 4 == 0, 16-byte aligned operands), 1: scalar rows
  int tile, S;                         // alpha: threads that span the channel groups, slices of L
  int nparts;                          // workgroups of the Gram launch
};

struct Layout { size_t xk, alphad, uu, kk, ga, gram, parts, total; };

Layout layout(long B, long C, long M) {
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  Layout l;
  l.xk = 0;
  l.alphad = up((size_t)(B * C) * 8);
  l.uu = l.alphad + up((size_t)(B * M) * 8);
  l.kk = l.uu + up((size_t)(B * M) * 8);
  l.ga = l.kk + up((size_t)M * 8);
  l.gram = l.ga + up((size_t)(B * M) * 8);
  l.parts = l.gram + up((size_t)(3 * M * M) * 8);
  l.total = l.parts + up((size_t)MAX_GRID * 8);
  return l;
}

// All sums run in fp64 and are rounded to fp32 once, where a value leaves the kernel (see prompt.hip: the cost here is
// launches and round trips, not flops).  Sum over the wavefront in a fixed butterfly order, in every lane (all 64 active).
__device__ __forceinline__ double wave_sum_d(double v) {
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
  return v;
}

// sum over the workgroup in a fixed order (lanes, then waves 0, 1, ...), in every thread; NW waves, all threads call it
template <int NW>
__device__ __forceinline__ double block_sum(double v, double* s_red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_red[0];
  for (int w = 1; w < NW; ++w) t = t + s_red[w];
  return t;
}

__device__ __forceinline__ void ldv(const float* __restrict__ p, int vec, float e[4]) {
  if (vec == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
  } else {
    e[0] = p[0];
  }
}

__device__ __forceinline__ void stv(float* __restrict__ p, int vec, const double a[4]) {
  if (vec == 4) *reinterpret_cast<float4*>(p) = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]);
  else p[0] = (float)a[0];
}

// <p, q> over n floats (n % vec == 0), lanes strided, fp64, in every lane
__device__ __forceinline__ double wave_dot(const float* __restrict__ p, const float* __restrict__ q, long n, int vec, int lane) {
  double d = 0.0;
  for (long c = (long)lane * vec; c < n; c += 64 * vec) {
    float e[4], g[4];
    ldv(p + c, vec, e);
    ldv(q + c, vec, g);
    for (int i = 0; i < vec; ++i) d = d + (double)e[i] * (double)g[i];
  }
  return wave_sum_d(d);
}

__global__ __launch_bounds__(ST) void coda_alpha_kernel(CodaArgs a) {
  __shared__ double s_part[ST * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, C = a.C, L = a.L, M = a.M;
  double* xk = a.xk + (long)b * C;

  // ---- (1) the query xk[b] (workspace, fp64)
  {
    const int vec = a.vec, G = C / vec, tile = a.tile;
    const int sl = tid / tile, gl = tid - sl * tile;
    const int l0 = (int)((long)sl * L / a.S), l1 = (int)((long)(sl + 1) * L / a.S);      // S <= L: no slice is empty
    const float* xb = a.x + (long)b * L * C;
    for (int g0 = 0; g0 < G; g0 += tile) {                                              // workgroup-uniform
      const int g = g0 + gl;
      const bool mine = sl < a.S && g < G;
      double sum[4] = {0.0, 0.0, 0.0, 0.0};
      if (mine) {
        for (int l = l0; l < l1; ++l) {
          float e[4];
          ldv(xb + (long)l * C + (long)g * vec, vec, e);
          for (int i = 0; i < vec; ++i) sum[i] = sum[i] + (double)e[i];
        }
        const int o = (sl * tile + gl) * 4;                                             // (sl, gl) < (S, tile), S tile <= ST
        for (int i = 0; i < vec; ++i) s_part[o + i] = sum[i];
      }
      __syncthreads();
      if (mine && sl == 0)
        for (int i = 0; i < vec; ++i) {
          double t = sum[i];
          for (int q = 1; q < a.S; ++q) t = t + s_part[(q * tile + gl) * 4 + i];          // slices in order
          xk[g * vec + i] = t / (double)L;
        }
      __syncthreads();                                                                  // (also publishes xk to the workgroup)
    }
  }

  // ---- (2) one wave per component
  for (int m = wave; m < a.f; m += SW) {                                                // wave-uniform
    const float* ar = a.attn + (long)m * C;
    const float* kr = a.key + (long)m * C;
    double uu = 0.0, kk = 0.0, uk = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double u = xk[c] * (double)ar[c], k = (double)kr[c];
      uu = uu + u * u;
      kk = kk + k * k;
      uk = uk + u * k;
    }
    uu = wave_sum_d(uu);
    kk = wave_sum_d(kk);
    uk = wave_sum_d(uk);
    if (lane == 0) {
      const double al = uk / (fmax(sqrt(uu), NORM_EPS) * fmax(sqrt(kk), NORM_EPS));     // u == 0: an exact 0
      a.alpha[(long)b * M + m] = (float)al;
      a.alphad[(long)b * M + m] = al;
      a.uu[(long)b * M + m] = uu;
      if (b == 0) a.kk[m] = kk;
    }
  }
  for (int m = a.f + tid; m < M; m += ST) a.alpha[(long)b * M + m] = 0.0f;
}

__global__ __launch_bounds__(RT) void coda_gram_kernel(CodaArgs a) {
  __shared__ double s_w[RW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long ff = (long)a.f * a.f, total = 3 * ff;
  double part = 0.0;
  for (long e = (long)blockIdx.x * RW + wave; e < total; e += (long)gridDim.x * RW) {    // wave-uniform
    const int tz = (int)(e / ff);
    const long rem = e - tz * ff;
    const int i = (int)(rem / a.f), j = (int)(rem - (long)i * a.f);
    if (j < i) continue;                                                                // the lower triangle is the upper's
    const float* T = tz == 0 ? a.key : (tz == 1 ? a.attn : a.prompt);
    const long D = tz == 2 ? (long)a.len * a.C : (long)a.C;
    const double g = wave_dot(T + i * D, T + j * D, D, a.vec, lane) - (i == j ? 1.0 : 0.0);
    if (lane == 0) {
      a.gram[tz * ff + (long)i * a.f + j] = g;
      a.gram[tz * ff + (long)j * a.f + i] = g;
    }
    part = part + (i == j ? 1.0 : 2.0) * g * g;
  }
  if (lane == 0) s_w[wave] = part;
  __syncthreads();
  if (tid == 0) {
    double t = s_w[0];
    for (int w = 1; w < RW; ++w) t = t + s_w[w];
    a.parts[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(RT) void coda_mix_kernel(CodaArgs a) {
  __shared__ double s_red[RW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = a.C, vec = a.vec;
  if (blockIdx.x == 0) {                                                                // workgroup-uniform
    double v = 0.0;
    if (a.want_ortho)
      for (int i = tid; i < a.nparts; i += RT) v = v + a.parts[i];
    v = block_sum<RW>(v, s_red);
    if (tid == 0) a.ortho[0] = (float)(v / ((double)a.f * (double)a.f));
  }
  const long T = (long)a.len + a.L, rows = (long)a.B * T;
  for (long r = (long)blockIdx.x * RW + wave; r < rows; r += (long)gridDim.x * RW) {     // wave-uniform
    const long b = r / T, t = r - b * T;
    float* dst = a.prompted + r * C;
    if (t < a.len) {
      const double* al = a.alphad + b * a.M;
      for (int c = lane * vec; c < C; c += 64 * vec) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < a.f; ++m) {                                                 // in order of m
          float e[4];
          ldv(a.prompt + ((long)m * a.len + t) * C + c, vec, e);
          const double w = al[m];
          for (int i = 0; i < vec; ++i) acc[i] = acc[i] + w * (double)e[i];
        }
        stv(dst + c, vec, acc);
      }
    } else {
      const float* src = a.x + (b * a.L + (t - a.len)) * C;
      if (vec == 4) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int c = lane; c < C / 4; c += 64) d4[c] = s4[c];
      } else {
        for (int c = lane; c < C; c += 64) dst[c] = src[c];
      }
    }
  }
}

__global__ __launch_bounds__(RT) void coda_bwd_dot_kernel(CodaArgs a, const float* __restrict__ gp, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nm = a.f - a.s;
  const long T = (long)a.len + a.L, D = (long)a.len * a.C, pairs = (long)a.B * nm;
  for (long r = (long)blockIdx.x * RW + wave; r < pairs; r += (long)gridDim.x * RW) {    // wave-uniform
    const long b = r / nm;
    const int m = a.s + (int)(r - b * nm);
    const double d = wave_dot(gp + b * T * a.C, a.prompt + (long)m * D, D, vec, lane);
    if (lane == 0) a.ga[b * a.M + m] = d;
  }
}

__global__ __launch_bounds__(RT) void coda_bwd_rows_kernel(CodaArgs a, const float* __restrict__ gp, const float* __restrict__ g_ortho,
                                                           float* __restrict__ d_prompt, float* __restrict__ d_key,
                                                           float* __restrict__ d_attn, int vec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, M = a.M, f = a.f;
  const long T = (long)a.len + a.L, ff = (long)f * f;
  const long p_rows = d_prompt ? (long)M * a.len : 0, k_rows = (d_key || d_attn) ? (long)M : 0;
  const double go = a.want_ortho ? (double)g_ortho[0] * 4.0 / ((double)f * (double)f) : 0.0;
  const double zero[4] = {0.0, 0.0, 0.0, 0.0};
  for (long r = (long)blockIdx.x * RW + wave; r < p_rows + k_rows; r += (long)gridDim.x * RW) {      // wave-uniform
    if (r < p_rows) {
      const int m = (int)(r / a.len), t = (int)(r - (long)m * a.len);
      float* dst = d_prompt + r * C;
      const bool live = m >= a.s && m < f;
      for (int c = lane * vec; c < C; c += 64 * vec) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
          for (int b = 0; b < a.B; ++b) {                                               // in order of b
            float e[4];
            ldv(gp + ((long)b * T + t) * C + c, vec, e);
            const double w = a.alphad[(long)b * M + m];
            for (int i = 0; i < vec; ++i) acc[i] = acc[i] + w * (double)e[i];
          }
          if (a.want_ortho) {
            double pen[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < f; ++j) {
              float e[4];
              ldv(a.prompt + ((long)j * a.len + t) * C + c, vec, e);
              const double w = a.gram[2 * ff + (long)m * f + j];
              for (int i = 0; i < vec; ++i) pen[i] = pen[i] + w * (double)e[i];
            }
            for (int i = 0; i < vec; ++i) acc[i] = acc[i] + go * pen[i];
          }
        }
        stv(dst + c, vec, live ? acc : zero);
      }
    } else {
      const int m = (int)(r - p_rows);
      const bool live = m >= a.s && m < f;
      const double kq = live ? a.kk[m] : 1.0;
      const double sk = sqrt(kq), nk = fmax(sk, NORM_EPS);
      const bool free_k = sk >= NORM_EPS;                                               // clamp_min passes the gradient at equality
      for (int c = lane * vec; c < C; c += 64 * vec) {
        double dk[4] = {0.0, 0.0, 0.0, 0.0}, da[4] = {0.0, 0.0, 0.0, 0.0};
        if (live) {
          float K[4], A[4];
          ldv(a.key + (long)m * C + c, vec, K);
          ldv(a.attn + (long)m * C + c, vec, A);
          for (int b = 0; b < a.B; ++b) {                                               // in order of b
            const double su = sqrt(a.uu[(long)b * M + m]), nu = fmax(su, NORM_EPS);
            const bool free_u = su >= NORM_EPS;
            const double al = a.alphad[(long)b * M + m], g = a.ga[(long)b * M + m];
            for (int i = 0; i < vec; ++i) {
              const double xkc = a.xk[(long)b * C + c + i];
              const double uh = xkc * (double)A[i] / nu, kh = (double)K[i] / nk;
              dk[i] = dk[i] + g * ((free_k ? uh - al * kh : uh) / nk);
              da[i] = da[i] + g * xkc * ((free_u ? kh - al * uh : kh) / nu);
            }
          }
          if (a.want_ortho) {
            double pk[4] = {0.0, 0.0, 0.0, 0.0}, pa[4] = {0.0, 0.0, 0.0, 0.0};
            for (int j = 0; j < f; ++j) {
              float e[4], h[4];
              ldv(a.key + (long)j * C + c, vec, e);
              ldv(a.attn + (long)j * C + c, vec, h);
              const double wk = a.gram[(long)m * f + j], wa = a.gram[ff + (long)m * f + j];
              for (int i = 0; i < vec; ++i) { pk[i] = pk[i] + wk * (double)e[i]; pa[i] = pa[i] + wa * (double)h[i]; }
            }
            for (int i = 0; i < vec; ++i) { dk[i] = dk[i] + go * pk[i]; da[i] = da[i] + go * pa[i]; }
          }
        }
        if (d_key) stv(d_key + (long)m * C + c, vec, dk);
        if (d_attn) stv(d_attn + (long)m * C + c, vec, da);
      }
    }
  }
}

// everything a launch relies on, checked on the host before any device work
int check_desc(const vilco_coda_desc* d) {
  if (!d) return VILCO_ERR_BADARG;
  if (d->B < 1 || d->L < 1 || d->C < 1 || d->len < 1) return VILCO_ERR_BADARG;
  if (!(1 <= d->f && d->f <= d->M && d->M <= MAX_M)) return VILCO_ERR_BADARG;
  if (!(0 <= d->s && d->s < d->f)) return VILCO_ERR_BADARG;
  if (!d->x || !d->prompt || !d->key || !d->attn || !d->alpha || !d->prompted || !d->ortho) return VILCO_ERR_BADARG;
  if (!d->workspace || !vilco_aligned(d->workspace, 256)) return VILCO_ERR_BADARG;
  if (d->workspace_bytes < layout(d->B, d->C, d->M).total) return VILCO_ERR_WORKSPACE;
  return VILCO_OK;
}

int row_grid(long rows) {
  const long g = (rows + RW - 1) / RW;
  return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

CodaArgs make_args(const vilco_coda_desc* d) {
  CodaArgs a;
  a.x = d->x; a.prompt = d->prompt; a.key = d->key; a.attn = d->attn;
  a.alpha = d->alpha; a.prompted = d->prompted; a.ortho = d->ortho;
  const Layout l = layout(d->B, d->C, d->M);
  unsigned char* w = reinterpret_cast<unsigned char*>(d->workspace);
  a.xk = reinterpret_cast<double*>(w + l.xk);
  a.alphad = reinterpret_cast<double*>(w + l.alphad);
  a.uu = reinterpret_cast<double*>(w + l.uu);
  a.kk = reinterpret_cast<double*>(w + l.kk);
  a.ga = reinterpret_cast<double*>(w + l.ga);
  a.gram = reinterpret_cast<double*>(w + l.gram);
  a.parts = reinterpret_cast<double*>(w + l.parts);
  a.B = d->B; a.L = d->L; a.C = d->C; a.M = d->M; a.len = d->len; a.s = d->s; a.f = d->f;
  a.want_ortho = d->want_ortho != 0;
  a.vec = (d->C % 4 == 0 && vilco_aligned(d->x, 16) && vilco_aligned(d->prompt, 16) && vilco_aligned(d->key, 16) &&
           vilco_aligned(d->attn, 16) && vilco_aligned(d->prompted, 16)) ? 4 : 1;
  const int G = d->C / a.vec, full = (G + 63) / 64 * 64;
  a.tile = full < ST ? full : ST;
  a.S = ST / a.tile < d->L ? ST / a.tile : d->L;
  a.nparts = row_grid(3L * d->f * d->f);
  return a;
}

}  // namespace

extern "C" size_t vilco_coda_workspace(const vilco_coda_desc* d) {
  if (!d || d->B < 1 || d->C < 1 || d->M < 1) return 0;
  return layout(d->B, d->C, d->M).total;
}

extern "C" int vilco_coda_fwd(const vilco_coda_desc* d, void* stream) {
  const int rc = check_desc(d);
  if (rc != VILCO_OK) return rc;
  const CodaArgs a = make_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(coda_alpha_kernel, dim3(d->B), dim3(ST), 0, s, a);
  if (a.want_ortho) hipLaunchKernelGGL(coda_gram_kernel, dim3(a.nparts), dim3(RT), 0, s, a);
  hipLaunchKernelGGL(coda_mix_kernel, dim3(row_grid((long)d->B * ((long)d->len + d->L))), dim3(RT), 0, s, a);
  return vilco_launch_status();
}

extern "C" int vilco_coda_bwd(const vilco_coda_desc* d, const float* g_prompted, const float* g_ortho, float* d_prompt,
                              float* d_key, float* d_attn, void* stream) {
  const int rc = check_desc(d);
  if (rc != VILCO_OK) return rc;
  if (!g_prompted || (d->want_ortho && !g_ortho)) return VILCO_ERR_BADARG;
  if (!d_prompt && !d_key && !d_attn) return VILCO_OK;
  const CodaArgs a = make_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int vec = (a.vec == 4 && vilco_aligned(g_prompted, 16) && (!d_prompt || vilco_aligned(d_prompt, 16)) &&
                   (!d_key || vilco_aligned(d_key, 16)) && (!d_attn || vilco_aligned(d_attn, 16))) ? 4 : 1;
  if (d_key || d_attn)
    hipLaunchKernelGGL(coda_bwd_dot_kernel, dim3(row_grid((long)d->B * (d->f - d->s))), dim3(RT), 0, s, a, g_prompted, vec);
  const long rows = (d_prompt ? (long)d->M * d->len : 0) + ((d_key || d_attn) ? (long)d->M : 0);
  hipLaunchKernelGGL(coda_bwd_rows_kernel, dim3(row_grid(rows)), dim3(RT), 0, s, a, g_prompted, g_ortho, d_prompt, d_key, d_attn, vec);
  return vilco_launch_status();
}
