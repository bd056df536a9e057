// Elastic Response Distillation (Feng, Wang, Yuan: "Overcoming Catastrophic Forgetting in Incremental Object Detection via
// Elastic Response Distillation", CVPR 2022; the reference has no method that holds the regression head, so there is no line of
// it to cite): at the positions where the model that ENTERS a task answers with statistical confidence on a clip, the new
// model's logits and boundary offsets are held to the old ones.  The definition is the float64 restatement
// tests/erd_restatement.py, not the paper's GFL-specific form (DESIGN.md 3.23 lists the departures).
//
// Record time (vilco_erd_select / vilco_erd_select_fill; z = the incoming model's logits [B][P][C], levels end to end,
// o^ = its finished offsets [B][P][2], V = the positions below their level's valid length):
//   c_i = max_{y < n_old} z_iy;  mu = mean_V c;  sigma = sqrt(mean_V (c - mu)^2)        (fp64, two passes, fixed order)
//   S_cls = {i in V: c_i > mu + alpha_cls sigma};  S_reg = {i in V: c_i > mu + alpha_reg sigma and o^_i0 + o^_i1 > 0}
//   erd_conf_kernel    one wavefront per row: c_i.
//   erd_stats_kernel   one workgroup per clip: mu, sigma, a flag word per position, |S_cls| and |S_reg|.
//   erd_fill_kernel    one workgroup per clip: the two maps position -> slot (-1: not selected) by a ballot / prefix scan in
//                      ascending position, then the selected rows gathered.  No atomic decides a slot.
//
// Every step (vilco_erd_fwd / _bwd; x = the concatenated head output [B][R][C], o = the offsets [B][R][2] -- finished, or raw
// with the per-level Scale: o = relu(fl32(scale_l raw)); everything per batch read through erd_tab):
//   A = sum_b sum_{i in S_cls(b)} sum_{y < n_b} (x_iy - z_iy)^2      N_c = sum_b |S_cls(b)| n_b
//   D = sum_b sum_{i in S_reg(b)} diou(o_i, o^_i)                    N_r = sum_b |S_reg(b)|
//   out = (lambda_cls A / N_c + lambda_reg D / N_r, its first part, its second part); a part whose count is 0 is 0
//   diou(p, g) = 1 - I / max(U, eps) + (rho / max(len, eps))^2, I = min(p0, g0) + min(p1, g1), U = (p0 + p1) + (g0 + g1) - I,
//   len = max(p0, g0) + max(p1, g1), rho = (p1 - p0 - g1 + g0) / 2, eps = 1e-8: modeling/losses.py ctr_diou_loss_1d.  Its
//   gradient takes autograd's choices: a tie of min / max gives each side half, a clamp passes the gradient at >= eps.
//   All terms are formed in fp64 from the fp32 inputs and every output is rounded to fp32 once.
//   erd_rows_kernel    one wavefront per (batch row, pyramid row) pair (a block's four waves walk pairs w, w + 4 gridDim.x, ...);
//                      per block one partial of A, D, the two counts and the unweighted d scale_l, added in wave order.
//   erd_finish_kernel  one workgroup adds the partials in block order (fixed tree) and writes the losses, N_c, N_r, d scale.
//   erd_bwd_kernel     one wavefront per row of [B][R]: EVERY element of d_logits and d_offsets is assigned -- zeros on
//                      separator rows, unselected positions, classes >= n_b and when a count is 0; block 0 writes d_scale.
// Two launches forward, one backward, whatever B, L and the table; the grids depend on shapes only.  No atomics: the same
// bits on every call.
#include "common.h"

namespace {

constexpr int ET = 256;                // threads per workgroup (4 waves)
constexpr int WPB = ET / 64;
constexpr int MAX_BLOCKS = 1024;
constexpr int ERD_MAX_L = 16;
constexpr int PS = 4 + ERD_MAX_L;      // doubles of one block's partial: A, D, rows x n_b compared, rows regressed, d scale_l
constexpr int TAB_K = 5;               // erd_tab columns: map_cls, map_reg, val_cls, val_reg, n_b
constexpr double DIOU_EPS = 1e-8;

struct ErdArgs {
  const float* logits;
  const float* offsets;
  const float* scale;                  // [L] or null
  const int32_t* level_dev;            // [2][L]: first rows, lengths
  const int32_t* level_len;            // [B][L]
  const int64_t* tab;                  // [B][TAB_K]
  long rows;                           // sum of level_T
  long pairs;                          // B * rows
  int B, R, C, L;
};

struct ErdWs {                         // the workspace, from its first 256-byte boundary
  int64_t* count;                      // N_c, N_r
  double* ds;                          // [ERD_MAX_L]: sum of d diou / d scale_l, unweighted
  double* part;                        // [blocks][PS]
};

int grid_blocks(long pairs) {
  const long g = (pairs + WPB - 1) / WPB;
  return (int)(g < 1 ? 1 : (g > MAX_BLOCKS ? MAX_BLOCKS : g));
}

size_t ws_bytes(long pairs) { return 256 + 256 + (size_t)grid_blocks(pairs) * PS * sizeof(double); }

ErdWs ws_view(void* workspace) {
  unsigned char* u = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  ErdWs w;
  w.count = reinterpret_cast<int64_t*>(u);
  w.ds = reinterpret_cast<double*>(u + 16);
  w.part = reinterpret_cast<double*>(u + 256);
  return w;
}

__device__ __forceinline__ double wave_sum_f64(double v) {     // fixed butterfly, result in every lane
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup in a fixed tree; the result in every thread.  `sd` has ET entries.
__device__ __forceinline__ double block_sum_f64(double v, double* sd) {
  const int tid = threadIdx.x;
  __syncthreads();                                             // sd may still be read from the previous call
  sd[tid] = v;
  __syncthreads();
  for (int o = ET / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  return sd[0];
}

// what a selected position of a row compares: slots in the record's value buffers (-1: not in the set)
struct ErdRow {
  const float* zc;                     // the record's n_b logits of the position (sc >= 0)
  const float* zr;                     // the record's two offsets (sr >= 0)
  int sc, sr, nb, level;
};

// the record of batch row b at position n = first_l + t of level l, if the row has one and t is below the valid length
__device__ __forceinline__ bool lookup(const ErdArgs& a, long b, int l, long t, long n, ErdRow* r) {
  const int64_t* e = a.tab + b * TAB_K;
  const int64_t mc = e[0], mr = e[1], vc = e[2], vr = e[3], nb = e[4];
  if (mc == 0 || mr == 0 || vc == 0 || vr == 0 || nb < 1 || nb > a.C) return false;      // no record, or one not to be trusted
  if (t >= (long)a.level_len[b * a.L + l]) return false;
  r->sc = reinterpret_cast<const int32_t*>(mc)[n];
  r->sr = reinterpret_cast<const int32_t*>(mr)[n];
  r->nb = (int)nb;
  r->level = l;
  r->zc = reinterpret_cast<const float*>(vc) + (long)(r->sc < 0 ? 0 : r->sc) * nb;
  r->zr = reinterpret_cast<const float*>(vr) + (long)(r->sr < 0 ? 0 : r->sr) * 2;
  return r->sc >= 0 || r->sr >= 0;
}

// pair p of [B][sum T_l] -> the row of x / o it names (element offset of its first logit / C) and its record
__device__ __forceinline__ bool locate_pair(const ErdArgs& a, long p, long* xrow, ErdRow* r) {
  const long b = p / a.rows, n = p - b * a.rows;
  long first = 0;
  for (int l = 0; l < a.L; ++l) {
    const int T = a.level_dev[a.L + l];
    if (T <= 0) return false;
    if (n < first + T) {
      const long t = n - first, row = (long)a.level_dev[l] + t;
      if (a.level_dev[l] < 0 || row >= a.R) return false;      // the device table disagrees with the validated bounds
      *xrow = b * a.R + row;
      return lookup(a, b, l, t, n, r);
    }
    first += T;
  }
  return false;
}

// row q of [B][R] -> its record, if the row belongs to a level
__device__ __forceinline__ bool locate_row(const ErdArgs& a, long q, ErdRow* r) {
  const long b = q / a.R, row = q - b * a.R;
  long first = 0;
  for (int l = 0; l < a.L; ++l) {
    const int r0 = a.level_dev[l], T = a.level_dev[a.L + l];
    if (T <= 0 || r0 < 0) return false;
    if (row >= r0 && row < (long)r0 + T) return lookup(a, b, l, row - r0, first + (row - r0), r);
    first += T;
  }
  return false;
}

struct Diou { double loss, d0, d1; };

// ctr_diou_loss_1d(p, g) and its gradient in p, with autograd's choices at the ties and at the clamps
__device__ __forceinline__ Diou diou(double p0, double p1, double g0, double g1) {
  const double m0 = p0 < g0 ? 1.0 : (p0 == g0 ? 0.5 : 0.0);     // d min(p0, g0) / d p0; d max(p0, g0) / d p0 = 1 - m0
  const double m1 = p1 < g1 ? 1.0 : (p1 == g1 ? 0.5 : 0.0);
  const double inter = (p1 < g1 ? p1 : g1) + (p0 < g0 ? p0 : g0);
  const double un = (p0 + p1) + (g0 + g1) - inter;
  const double U = un > DIOU_EPS ? un : DIOU_EPS;
  const double pu = un >= DIOU_EPS ? 1.0 : 0.0;
  const double len = (p0 > g0 ? p0 : g0) + (p1 > g1 ? p1 : g1);
  const double Lc = len > DIOU_EPS ? len : DIOU_EPS;
  const double pc = len >= DIOU_EPS ? 1.0 : 0.0;
  const double rho = 0.5 * (p1 - p0 - g1 + g0);
  const double q = rho / Lc;
  Diou r;
  r.loss = 1.0 - inter / U + q * q;
  const double dU = inter / (U * U) * pu, dL = rho / (Lc * Lc) * pc;
  r.d0 = -(m0 / U - dU * (1.0 - m0)) + 2.0 * q * (-0.5 / Lc - dL * (1.0 - m0));
  r.d1 = -(m1 / U - dU * (1.0 - m1)) + 2.0 * q * (0.5 / Lc - dL * (1.0 - m1));
  return r;
}

// the student's offsets of a row: finished, or relu(fl32(scale_l raw)) -- `keep` = 1 where the relu passes the gradient
__device__ __forceinline__ void student(const ErdArgs& a, long xrow, int level, float* o, float* raw, float* keep, float* s) {
  raw[0] = a.offsets[xrow * 2];
  raw[1] = a.offsets[xrow * 2 + 1];
  if (a.scale) {
    *s = a.scale[level];
    for (int k = 0; k < 2; ++k) {
      const float pre = raw[k] * *s;
      keep[k] = pre > 0.f ? 1.f : 0.f;
      o[k] = pre > 0.f ? pre : 0.f;
    }
  } else {
    *s = 1.f;
    o[0] = raw[0]; o[1] = raw[1];
    keep[0] = keep[1] = 1.f;
  }
}

__global__ __launch_bounds__(ET) void erd_rows_kernel(ErdArgs a, double* __restrict__ part) {
  __shared__ double sw[WPB][PS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = lane; i < PS; i += 64) sw[wave][i] = 0.0;       // a wave's own row: only that wave touches it
  double accA = 0.0, accD = 0.0, cntc = 0.0, cntr = 0.0;       // (counts below 2^53: exact in a double)
  for (long p = (long)blockIdx.x * WPB + wave; p < a.pairs; p += (long)gridDim.x * WPB) {      // wave-uniform
    ErdRow r;
    long xrow = 0;
    if (!locate_pair(a, p, &xrow, &r)) continue;
    if (r.sc >= 0) {
      const float* x = a.logits + xrow * a.C;
      double v = 0.0;
      for (int y = lane; y < r.nb; y += 64) {
        const double d = (double)x[y] - (double)r.zc[y];
        v = v + d * d;
      }
      accA = accA + wave_sum_f64(v);
      cntc = cntc + (double)r.nb;
    }
    if (r.sr >= 0) {                                           // every lane forms the same two-number term
      float o[2], raw[2], keep[2], s;
      student(a, xrow, r.level, o, raw, keep, &s);
      const Diou t = diou((double)o[0], (double)o[1], (double)r.zr[0], (double)r.zr[1]);
      accD = accD + t.loss;
      cntr = cntr + 1.0;
      if (a.scale && lane == 0)
        sw[wave][4 + r.level] = sw[wave][4 + r.level] + (t.d0 * (double)(keep[0] * raw[0]) + t.d1 * (double)(keep[1] * raw[1]));
    }
  }
  if (lane == 0) {
    sw[wave][0] = accA; sw[wave][1] = accD; sw[wave][2] = cntc; sw[wave][3] = cntr;
  }
  __syncthreads();
  if (threadIdx.x < PS) {
    double v = sw[0][threadIdx.x];
    for (int k = 1; k < WPB; ++k) v = v + sw[k][threadIdx.x];
    part[(long)blockIdx.x * PS + threadIdx.x] = v;
  }
}

__global__ __launch_bounds__(ET) void erd_finish_kernel(const double* __restrict__ part, int nblk, double lambda_cls,
                                                        double lambda_reg, float* __restrict__ out, int64_t* __restrict__ count,
                                                        double* __restrict__ ds) {
  __shared__ double sd[ET];
  __shared__ double tot[PS];
  const int tid = threadIdx.x;
  for (int k = 0; k < PS; ++k) {
    double v = 0.0;
    for (int b = tid; b < nblk; b += ET) v = v + part[(long)b * PS + k];
    v = block_sum_f64(v, sd);
    if (tid == 0) tot[k] = v;
  }
  __syncthreads();
  if (tid < ERD_MAX_L) ds[tid] = tot[4 + tid];
  if (tid == 0) {
    const double nc = tot[2], nr = tot[3];
    const double cls = nc > 0.0 ? lambda_cls * tot[0] / nc : 0.0;
    const double reg = nr > 0.0 ? lambda_reg * tot[1] / nr : 0.0;
    count[0] = (int64_t)nc;
    count[1] = (int64_t)nr;
    out[0] = (float)(cls + reg);
    out[1] = (float)cls;
    out[2] = (float)reg;
  }
}

__global__ __launch_bounds__(ET) void erd_bwd_kernel(ErdArgs a, double lambda_cls, double lambda_reg, const float* __restrict__ g_out,
                                                     const int64_t* __restrict__ count, const double* __restrict__ ds,
                                                     float* __restrict__ d_logits, float* __restrict__ d_offsets,
                                                     float* __restrict__ d_scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t Nc = count[0], Nr = count[1];
  const double g = (double)g_out[0];
  const double cc = Nc > 0 ? 2.0 * lambda_cls * g / (double)Nc : 0.0;
  const double cr = Nr > 0 ? lambda_reg * g / (double)Nr : 0.0;
  if (blockIdx.x == 0 && d_scale && threadIdx.x < a.L) d_scale[threadIdx.x] = Nr > 0 ? (float)(cr * ds[threadIdx.x]) : 0.f;
  const long nrows = (long)a.B * a.R;
  for (long q = (long)blockIdx.x * WPB + wave; q < nrows; q += (long)gridDim.x * WPB) {      // wave-uniform
    ErdRow r;
    const bool has = locate_row(a, q, &r);
    const bool cmp = has && r.sc >= 0 && Nc > 0, regr = has && r.sr >= 0 && Nr > 0;
    const float* x = a.logits + q * a.C;
    float* d = d_logits + q * a.C;
    for (int y = lane; y < a.C; y += 64)
      d[y] = (cmp && y < r.nb) ? (float)(((double)x[y] - (double)r.zc[y]) * cc) : 0.f;
    float go[2] = {0.f, 0.f};
    if (regr) {
      float o[2], raw[2], keep[2], s;
      student(a, q, r.level, o, raw, keep, &s);
      const Diou t = diou((double)o[0], (double)o[1], (double)r.zr[0], (double)r.zr[1]);
      go[0] = keep[0] != 0.f ? (float)(t.d0 * cr * (double)s) : 0.f;
      go[1] = keep[1] != 0.f ? (float)(t.d1 * cr * (double)s) : 0.f;
    }
    if (lane < 2) d_offsets[q * 2 + lane] = lane == 0 ? go[0] : go[1];
  }
}

// everything a launch relies on, checked on the host; rows = sum of level_T on success
int check_desc(const vilco_erd_desc* d, long* rows) {
  if (!d || !d->logits || !d->offsets || !d->level_row || !d->level_T || !d->level_dev || !d->level_len || !d->erd_tab)
    return VILCO_ERR_BADARG;
  if (d->L <= 0 || d->L > ERD_MAX_L || d->B <= 0 || d->R < 1 || d->C < 1) return VILCO_ERR_BADARG;
  long n = 0;
  for (int l = 0; l < d->L; ++l) {
    const long r = d->level_row[l], T = d->level_T[l];
    if (r < 0 || T < 1 || r + T > d->R) return VILCO_ERR_BADARG;
    n += T;
  }
  *rows = n;
  return VILCO_OK;
}

ErdArgs make_args(const vilco_erd_desc* d, long rows) {
  ErdArgs a;
  a.logits = d->logits; a.offsets = d->offsets; a.scale = d->scale;
  a.level_dev = d->level_dev; a.level_len = d->level_len; a.tab = d->erd_tab;
  a.rows = rows; a.pairs = (long)d->B * rows;
  a.B = d->B; a.R = d->R; a.C = d->C; a.L = d->L;
  return a;
}

// ------------------------------------------------------------------------------------------------- selection (record time)
struct SelLevels { int T[ERD_MAX_L]; };

// is position i of clip b below its level's valid length?
__device__ __forceinline__ bool sel_valid(const SelLevels& lv, int L, const int32_t* __restrict__ level_len, int b, int i) {
  int first = 0;
  for (int l = 0; l < L; ++l) {
    const int T = lv.T[l];
    if (i < first + T) {
      int V = level_len[b * L + l];
      V = V < 0 ? 0 : (V > T ? T : V);
      return i - first < V;
    }
    first += T;
  }
  return false;
}

__global__ __launch_bounds__(ET) void erd_conf_kernel(const float* __restrict__ z, long nrows, int C, int n_old,
                                                      float* __restrict__ conf) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long p = (long)blockIdx.x * WPB + wave; p < nrows; p += (long)gridDim.x * WPB) {      // wave-uniform
    const float* x = z + p * C;
    float m = -INFINITY;
    for (int y = lane; y < n_old; y += 64) m = fmaxf(m, x[y]);
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) conf[p] = m;
  }
}

__global__ __launch_bounds__(ET) void erd_stats_kernel(SelLevels lv, int L, int P, const int32_t* __restrict__ level_len,
                                                       const float* __restrict__ conf, const float* __restrict__ offsets,
                                                       double alpha_cls, double alpha_reg, int32_t* __restrict__ flags,
                                                       int32_t* __restrict__ counts) {
  __shared__ double sd[ET];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* c = conf + (long)b * P;
  const float* o = offsets + (long)b * P * 2;
  int32_t* f = flags + (long)b * P;
  double s = 0.0, n = 0.0;                                     // thread tid owns the positions tid, tid + ET, ... throughout
  for (int i = tid; i < P; i += ET) {
    if (sel_valid(lv, L, level_len, b, i)) { s = s + (double)c[i]; n = n + 1.0; }
  }
  s = block_sum_f64(s, sd);
  n = block_sum_f64(n, sd);
  if (n == 0.0) {                                              // block-uniform: a clip without a valid position
    for (int i = tid; i < P; i += ET) f[i] = 0;
    if (tid == 0) { counts[2 * b] = 0; counts[2 * b + 1] = 0; }
    return;
  }
  const double mu = s / n;
  double ss = 0.0;
  for (int i = tid; i < P; i += ET) {
    if (sel_valid(lv, L, level_len, b, i)) { const double e = (double)c[i] - mu; ss = ss + e * e; }
  }
  const double sigma = sqrt(block_sum_f64(ss, sd) / n);
  const double tc = mu + alpha_cls * sigma, tr = mu + alpha_reg * sigma;
  double kc = 0.0, kr = 0.0;
  for (int i = tid; i < P; i += ET) {
    int w = 0;
    if (sel_valid(lv, L, level_len, b, i)) {
      const double ci = (double)c[i];
      if (ci > tc) w |= 1;
      if (ci > tr && (double)o[2 * i] + (double)o[2 * i + 1] > 0.0) w |= 2;
    }
    f[i] = w;
    kc = kc + (double)(w & 1);
    kr = kr + (double)(w >> 1);
  }
  kc = block_sum_f64(kc, sd);
  kr = block_sum_f64(kr, sd);
  if (tid == 0) { counts[2 * b] = (int32_t)kc; counts[2 * b + 1] = (int32_t)kr; }
}

// out_tab [B][4]: the clip's map_cls [P], map_reg [P], val_cls [K_c][n_old], val_reg [K_r][2] -- K as erd_stats_kernel counted
__global__ __launch_bounds__(ET) void erd_fill_kernel(int P, int C, int n_old, const float* __restrict__ z,
                                                      const float* __restrict__ offsets, const int32_t* __restrict__ flags,
                                                      const int32_t* __restrict__ counts, const int64_t* __restrict__ out_tab) {
  __shared__ int wt[2][WPB];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* f = flags + (long)b * P;
  int32_t* map_c = reinterpret_cast<int32_t*>(out_tab[4 * b]);
  int32_t* map_r = reinterpret_cast<int32_t*>(out_tab[4 * b + 1]);
  float* val_c = reinterpret_cast<float*>(out_tab[4 * b + 2]);
  float* val_r = reinterpret_cast<float*>(out_tab[4 * b + 3]);
  const int Kc = counts[2 * b], Kr = counts[2 * b + 1];
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int base_c = 0, base_r = 0;
  for (int i0 = 0; i0 < P; i0 += ET) {                          // block-uniform: ascending position
    const int i = i0 + tid;
    const int w = i < P ? f[i] : 0;
    const unsigned long long mc = __ballot(w & 1), mr = __ballot((w >> 1) & 1);
    if (lane == 0) { wt[0][wave] = __popcll(mc); wt[1][wave] = __popcll(mr); }
    __syncthreads();
    int oc = base_c, orr = base_r, tc = 0, tr = 0;
    for (int k = 0; k < WPB; ++k) {
      if (k < wave) { oc += wt[0][k]; orr += wt[1][k]; }
      tc += wt[0][k]; tr += wt[1][k];
    }
    if (i < P) {
      const int sc = oc + __popcll(mc & below), sr = orr + __popcll(mr & below);
      map_c[i] = ((w & 1) && sc < Kc) ? sc : -1;                // (sc < K always: the flags are the ones that were counted)
      map_r[i] = ((w & 2) && sr < Kr) ? sr : -1;
    }
    base_c += tc; base_r += tr;
    __syncthreads();
  }
  for (int i = wave; i < P; i += WPB) {                         // the block's own writes, behind the barrier above
    const int sc = map_c[i], sr = map_r[i];
    const long src = (long)b * P + i;
    if (sc >= 0)
      for (int y = lane; y < n_old; y += 64) val_c[(long)sc * n_old + y] = z[src * C + y];
    if (sr >= 0 && lane < 2) val_r[(long)sr * 2 + lane] = offsets[src * 2 + lane];
  }
}

int check_select(const vilco_erd_select_desc* d, SelLevels* lv) {
  if (!d || !d->logits || !d->offsets || !d->level_T || !d->level_len || !d->conf || !d->flags || !d->counts)
    return VILCO_ERR_BADARG;
  if (d->L < 1 || d->L > ERD_MAX_L || d->B < 1 || d->P < 1 || d->C < 1 || d->n_old < 1 || d->n_old > d->C) return VILCO_ERR_BADARG;
  if (!(d->alpha_cls == d->alpha_cls) || !(d->alpha_reg == d->alpha_reg)) return VILCO_ERR_BADARG;
  long n = 0;
  for (int l = 0; l < ERD_MAX_L; ++l) {
    lv->T[l] = l < d->L ? d->level_T[l] : 0;
    if (l < d->L && d->level_T[l] < 1) return VILCO_ERR_BADARG;
    n += lv->T[l];
  }
  return n == d->P ? VILCO_OK : VILCO_ERR_BADARG;
}

}  // namespace

extern "C" int32_t vilco_erd_pairs_per_round(void) { return WPB * MAX_BLOCKS; }

extern "C" size_t vilco_erd_workspace(int64_t n_pairs) { return n_pairs < 0 ? 0 : ws_bytes(n_pairs); }

extern "C" int vilco_erd_fwd(const vilco_erd_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  long rows = 0;
  const int rc = check_desc(d, &rows);
  if (rc != VILCO_OK) return rc;
  if (!out || !workspace) return VILCO_ERR_BADARG;
  const ErdArgs a = make_args(d, rows);
  if (workspace_bytes < ws_bytes(a.pairs)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ErdWs w = ws_view(workspace);
  const int nblk = grid_blocks(a.pairs);
  hipLaunchKernelGGL(erd_rows_kernel, dim3(nblk), dim3(ET), 0, s, a, w.part);
  hipLaunchKernelGGL(erd_finish_kernel, dim3(1), dim3(ET), 0, s, (const double*)w.part, nblk, d->lambda_cls, d->lambda_reg, out,
                     w.count, w.ds);
  return vilco_launch_status();
}

extern "C" int vilco_erd_bwd(const vilco_erd_desc* d, const float* g_out, float* d_logits, float* d_offsets, float* d_scale,
                             const void* workspace, size_t workspace_bytes, void* stream) {
  long rows = 0;
  const int rc = check_desc(d, &rows);
  if (rc != VILCO_OK) return rc;
  if (!g_out || !d_logits || !d_offsets || !workspace || (d->scale && !d_scale)) return VILCO_ERR_BADARG;
  const ErdArgs a = make_args(d, rows);
  if (workspace_bytes < ws_bytes(a.pairs)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const ErdWs w = ws_view(const_cast<void*>(workspace));
  hipLaunchKernelGGL(erd_bwd_kernel, dim3(grid_blocks((long)d->B * d->R)), dim3(ET), 0, s, a, d->lambda_cls, d->lambda_reg, g_out,
                     (const int64_t*)w.count, (const double*)w.ds, d_logits, d_offsets, d->scale ? d_scale : nullptr);
  return vilco_launch_status();
}

extern "C" int vilco_erd_select(const vilco_erd_select_desc* d, void* stream) {
  SelLevels lv;
  const int rc = check_select(d, &lv);
  if (rc != VILCO_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long nrows = (long)d->B * d->P;
  hipLaunchKernelGGL(erd_conf_kernel, dim3(grid_blocks(nrows)), dim3(ET), 0, s, d->logits, nrows, (int)d->C, (int)d->n_old, d->conf);
  hipLaunchKernelGGL(erd_stats_kernel, dim3(d->B), dim3(ET), 0, s, lv, (int)d->L, (int)d->P, d->level_len, (const float*)d->conf,
                     d->offsets, d->alpha_cls, d->alpha_reg, d->flags, d->counts);
  return vilco_launch_status();
}

extern "C" int vilco_erd_select_fill(const vilco_erd_select_desc* d, void* stream) {
  SelLevels lv;
  const int rc = check_select(d, &lv);
  if (rc != VILCO_OK) return rc;
  if (!d->out_tab) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(erd_fill_kernel, dim3(d->B), dim3(ET), 0, s, (int)d->P, (int)d->C, (int)d->n_old, d->logits, d->offsets,
                     (const int32_t*)d->flags, (const int32_t*)d->counts, d->out_tab);
  return vilco_launch_status();
}
