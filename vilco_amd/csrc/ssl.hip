// Narration SSL of the ViLCo recipe on the device (MQ/libs/modeling/meta_archs.py:794-811 the two masked mean poolings,
// :38-60 the memory bank's ring update, :939-945 the branch of forward, :1351-1372 masked_contrastive_loss).
//
//   vilco_ssl_pool_fwd   out[b] = (1/L) sum_l (1/max(len_bl, 1)) sum_{t < len_bl} f_l[b, t, :] over a table of L token-major
//                        levels.  Workgroup (b, level, 32-row slab) adds its rows below the length in row order and writes a
//                        partial; a slab that starts at or above the length returns at once (nothing above the length is
//                        read).  A second launch adds every level's slabs in slab order, then the levels in level order, in
//                        fp64.  Every element below its length is read exactly once.
//   vilco_ssl_pool_bwd   dOut[b, :] / (L max(len, 1)) to the rows below the length, 0 above, one tensor per level.
//   vilco_ssl_nce_fwd    (1) L2-normalise the raw text and video rows (x / max(||x||, 1e-12)) and take the positive pairs'
//                        dot products; (2) ring update, a launch of its own: the normalised text rows with mask != 0,
//                        compacted in batch order, go to bank rows (ptr + rank) mod M and the ring word advances by their
//                        count; (3) logits of all 2B vectors against every bank row: a workgroup owns 16 bank rows, stages
//                        them through LDS once per 128 columns and uses that tile for every vector, writes the logits and a
//                        (max, sum exp) pair per vector; (4) one workgroup folds the pairs in chunk order with the positive
//                        logit into the log-sum-exp of every vector and adds the masked rows' terms in batch order.
//   vilco_ssl_nce_bwd    probabilities from the saved logits and log-sum-exps; dXn = P x bank split over (32 columns, slabs
//                        of bank rows), the slabs added in order by the launch that also adds the positive pair's cross term
//                        and applies the normalisation's Jacobian.
// fp32 data; the logits are accumulated and kept in fp64 (at temperature 0.07 a logit of 40 carries 4e-6 of fp32 rounding
// straight into its probability: more than the 1e-5 bar of this branch leaves room for), exponents are formed from fp64
// differences, partials are folded in fp64; fixed summation orders, no atomics, no allocation, no host
// synchronisation: a replayed launch sequence gives the bits of the eager one.  Nothing is divided by the count of masked
// rows when it is zero: loss and gradients are exact zeros, bank and ring word are not written.
#include "common.h"

namespace {

constexpr int ST = 256;                // threads per workgroup (4 waves)
constexpr int SSL_MAX_L = 16;
constexpr int POOL_ROWS = 32;          // rows of one level per pooling workgroup
constexpr int NCE_MAX_B = 64;
constexpr int NCE_MAX_D = 4096;
constexpr int NCE_JT = 16;             // bank rows per logits workgroup
constexpr int NCE_DT = 128;            // columns per staged tile
constexpr int NCE_LD = NCE_DT + 4;     // LDS row stride: 16-byte aligned rows, neighbouring rows 4 banks apart
constexpr int NCE_VT = 32;             // vectors per staged tile
constexpr int BW_DT = 32;              // columns per backward workgroup
constexpr int BW_JT = 32;              // bank rows per staged tile of the backward
constexpr int BW_MAX_SLABS = 8;
constexpr int RING_T = 1024;

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

struct PoolDims { int T[SSL_MAX_L]; int soff[SSL_MAX_L + 1]; };       // soff: first slab of every level, soff[L] = all slabs
struct PoolSrc { const float* p[SSL_MAX_L]; };
struct PoolDst { float* p[SSL_MAX_L]; };

__device__ __forceinline__ int pool_level(const PoolDims& dm, int L, int slab) {
  int l = 0;
  while (l + 1 < L && slab >= dm.soff[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ int pool_len(const int* __restrict__ lens, int b, int L, int l, int T) {
  const int n = lens[b * L + l];
  return n < 0 ? 0 : (n > T ? T : n);
}

// ---------------------------------------------------------------------------------------------------------------- pool
__global__ __launch_bounds__(ST) void ssl_pool_part_kernel(PoolSrc src, PoolDims dm, int L, const int* __restrict__ lens, int C,
                                                           int vec, float* __restrict__ part) {
  const int b = blockIdx.y, slab = blockIdx.x;
  const int l = pool_level(dm, L, slab);
  const int T = dm.T[l];
  const int len = pool_len(lens, b, L, l, T);
  const int t0 = (slab - dm.soff[l]) * POOL_ROWS;
  if (t0 >= len) return;                                       // the finishing launch stops at the length too
  const int t1 = t0 + POOL_ROWS < len ? t0 + POOL_ROWS : len;
  const float* f = src.p[l] + (long)b * T * C;
  float* out = part + ((long)b * dm.soff[L] + slab) * C;
  if (vec) {
    for (int c = threadIdx.x * 4; c < C; c += ST * 4) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = t0; t < t1; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(f + (long)t * C + c);
        a.x = a.x + v.x; a.y = a.y + v.y; a.z = a.z + v.z; a.w = a.w + v.w;
      }
      vilco_st_agent(out + c, a.x); vilco_st_agent(out + c + 1, a.y);
      vilco_st_agent(out + c + 2, a.z); vilco_st_agent(out + c + 3, a.w);
    }
  } else {
    for (int c = threadIdx.x; c < C; c += ST) {
      float a = 0.f;
      for (int t = t0; t < t1; ++t) a = a + f[(long)t * C + c];
      vilco_st_agent(out + c, a);
    }
  }
}

__global__ __launch_bounds__(ST) void ssl_pool_finish_kernel(const float* __restrict__ part, PoolDims dm, int L,
                                                             const int* __restrict__ lens, int C, float* __restrict__ out) {
  const int b = blockIdx.y, c = blockIdx.x * ST + threadIdx.x;
  if (c >= C) return;
  double acc = 0.0;
  for (int l = 0; l < L; ++l) {
    const int len = pool_len(lens, b, L, l, dm.T[l]);
    if (len == 0) continue;
    const int ns = (len + POOL_ROWS - 1) / POOL_ROWS;
    const float* p = part + ((long)b * dm.soff[L] + dm.soff[l]) * C + c;
    double s = 0.0;
    for (int k = 0; k < ns; ++k) s = s + (double)vilco_ld_agent(p + (long)k * C);
    acc = acc + s / (double)len;
  }
  out[(long)b * C + c] = (float)(acc / (double)L);
}

__global__ __launch_bounds__(ST) void ssl_pool_bwd_kernel(const float* __restrict__ dout, PoolDst dst, PoolDims dm, int L,
                                                          const int* __restrict__ lens, int C, int vec) {
  const int b = blockIdx.y, slab = blockIdx.x;
  const int l = pool_level(dm, L, slab);
  const int T = dm.T[l];
  const int len = pool_len(lens, b, L, l, T);
  const int t0 = (slab - dm.soff[l]) * POOL_ROWS;
  const int t1 = t0 + POOL_ROWS < T ? t0 + POOL_ROWS : T;
  const float scale = 1.0f / ((float)L * (float)(len > 0 ? len : 1));
  const float* g = dout + (long)b * C;
  float* d = dst.p[l] + (long)b * T * C;
  if (vec) {
    for (int c = threadIdx.x * 4; c < C; c += ST * 4) {
      float4 v = *reinterpret_cast<const float4*>(g + c);
      v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int t = t0; t < t1; ++t) *reinterpret_cast<float4*>(d + (long)t * C + c) = t < len ? v : z;
    }
  } else {
    for (int c = threadIdx.x; c < C; c += ST) {
      const float v = g[c] * scale;
      for (int t = t0; t < t1; ++t) d[(long)t * C + c] = t < len ? v : 0.f;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- nce
// sum over the workgroup in a fixed tree; the result in every thread.  `sd` has ST entries.
__device__ __forceinline__ float block_sum(float v, float* sd) {
  const int tid = threadIdx.x;
  __syncthreads();                                             // sd may still be read from the previous call
  sd[tid] = v;
  __syncthreads();
  for (int o = ST / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  return sd[0];
}

__device__ __forceinline__ int nce_count(const float* __restrict__ mask, int B) {
  int n = 0;
  for (int i = 0; i < B; ++i) n += mask[i] != 0.f ? 1 : 0;
  return n;
}

// workgroup b: xn[0][b] = text[b] / max(||text[b]||, eps), xn[1][b] likewise of video[b];
// stats = [norm 2B | pos B | lse shift 2B | log of the shifted sum 2B]: lse_v = stats[3B + v] + stats[5B + v]
__global__ __launch_bounds__(ST) void ssl_norm_kernel(const float* __restrict__ text, const float* __restrict__ video, int B, int D,
                                                      float* __restrict__ xn, float* __restrict__ stats) {
  __shared__ float sd[ST];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* t = text + (long)b * D;
  const float* v = video + (long)b * D;
  float st = 0.f, sv = 0.f;
  for (int d = tid; d < D; d += ST) { st = st + t[d] * t[d]; sv = sv + v[d] * v[d]; }
  const float nt = fmaxf(sqrtf(block_sum(st, sd)), 1e-12f);
  const float nv = fmaxf(sqrtf(block_sum(sv, sd)), 1e-12f);
  float* tn = xn + (long)b * D;
  float* vn = xn + ((long)B + b) * D;
  float pos = 0.f;
  for (int d = tid; d < D; d += ST) {
    const float a = t[d] / nt, c = v[d] / nv;
    tn[d] = a; vn[d] = c;
    pos = pos + a * c;
  }
  pos = block_sum(pos, sd);
  if (tid == 0) { stats[b] = nt; stats[B + b] = nv; stats[2 * B + b] = pos; }
}

// one workgroup: rows[b] with mask[b] != 0 -> bank[(ptr + rank) mod M], then ring word = (ptr + n) mod M (n > 0 only)
__global__ __launch_bounds__(RING_T) void ssl_ring_kernel(const float* __restrict__ rows, const float* __restrict__ mask, int B,
                                                          int D, float* __restrict__ bank, int M, int* __restrict__ ring) {
  __shared__ int rank[NCE_MAX_B];
  __shared__ int n_s, p_s;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int p = ring[0] % M;
    if (p < 0) p += M;
    int n = 0;
    for (int b = 0; b < B; ++b) rank[b] = mask[b] != 0.f ? n++ : -1;
    n_s = n; p_s = p;
  }
  __syncthreads();
  const int n = n_s, p = p_s, D4 = D >> 2;
  if (n == 0) return;
  const float4* src = reinterpret_cast<const float4*>(rows);
  float4* dst = reinterpret_cast<float4*>(bank);
  for (int idx = tid; idx < B * D4; idx += RING_T) {
    const int b = idx / D4, q = idx - b * D4;
    if (rank[b] >= 0) dst[(long)((p + rank[b]) % M) * D4 + q] = src[idx];
  }
  if (tid == 0) ring[0] = (p + n) % M;
}

// workgroup = NCE_JT bank rows against all V = 2B vectors.  Thread (tv = tid / 16, tj = tid % 16) owns bank row tj and the
// vectors tv, tv + 16 of every tile of 32 vectors.
__global__ __launch_bounds__(ST) void ssl_logits_kernel(const float* __restrict__ xn, const float* __restrict__ bank, int V, int D,
                                                        int M, float tau, double* __restrict__ logits, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Bs[NCE_JT * NCE_LD];
  __shared__ __attribute__((aligned(16))) float Xs[NCE_VT * NCE_LD];
  __shared__ double Ls[2 * NCE_MAX_B][NCE_JT + 1];
  const int tid = threadIdx.x, tj = tid & 15, tv = tid >> 4;
  const int j0 = blockIdx.x * NCE_JT, nchunk = gridDim.x;
  const int nvt = (V + NCE_VT - 1) / NCE_VT;
  double acc[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a) { acc[a][0] = 0.0; acc[a][1] = 0.0; }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int d0 = 0; d0 < D; d0 += NCE_DT) {
    __syncthreads();                                           // the previous tiles have been consumed
#pragma unroll
    for (int q = 0; q < NCE_JT * (NCE_DT / 4) / ST; ++q) {
      const int idx = tid + q * ST, r = idx >> 5, c = (idx & 31) * 4;
      const int j = j0 + r, d = d0 + c;
      *reinterpret_cast<float4*>(&Bs[r * NCE_LD + c]) =
          (j < M && d < D) ? *reinterpret_cast<const float4*>(bank + (long)j * D + d) : z4;
    }
#pragma unroll
    for (int vt = 0; vt < 4; ++vt) {
      if (vt < nvt) {
        if (vt) __syncthreads();                               // the previous vector tile has been consumed
#pragma unroll
        for (int q = 0; q < NCE_VT * (NCE_DT / 4) / ST; ++q) {
          const int idx = tid + q * ST, r = idx >> 5, c = (idx & 31) * 4;
          const int v = vt * NCE_VT + r, d = d0 + c;
          *reinterpret_cast<float4*>(&Xs[r * NCE_LD + c]) =
              (v < V && d < D) ? *reinterpret_cast<const float4*>(xn + (long)v * D + d) : z4;
        }
        __syncthreads();
        double a0 = acc[vt][0], a1 = acc[vt][1];
#pragma unroll 8
        for (int k = 0; k < NCE_DT; k += 4) {
          const float4 bb = *reinterpret_cast<const float4*>(&Bs[tj * NCE_LD + k]);
          const float4 x0 = *reinterpret_cast<const float4*>(&Xs[tv * NCE_LD + k]);
          const float4 x1 = *reinterpret_cast<const float4*>(&Xs[(tv + 16) * NCE_LD + k]);
          const double bx = bb.x, by = bb.y, bz = bb.z, bw = bb.w;
          a0 = fma((double)x0.x, bx, a0); a0 = fma((double)x0.y, by, a0); a0 = fma((double)x0.z, bz, a0); a0 = fma((double)x0.w, bw, a0);
          a1 = fma((double)x1.x, bx, a1); a1 = fma((double)x1.y, by, a1); a1 = fma((double)x1.z, bz, a1); a1 = fma((double)x1.w, bw, a1);
        }
        acc[vt][0] = a0; acc[vt][1] = a1;
      }
    }
  }
  const double ninf = -__builtin_huge_val();
  const int j = j0 + tj;
#pragma unroll
  for (int vt = 0; vt < 4; ++vt) {
    if (vt < nvt) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int v = vt * NCE_VT + tv + 16 * h;
        if (v < V) {
          const double lg = acc[vt][h] / (double)tau;
          if (j < M) logits[(long)v * M + j] = lg;
          Ls[v][tj] = j < M ? lg : ninf;
        }
      }
    }
  }
  __syncthreads();
  if (tid < V) {                                               // (the chunk's first row always exists: the maximum is finite)
    double md = Ls[tid][0];
    for (int k = 1; k < NCE_JT; ++k) md = fmax(md, Ls[tid][k]);
    const float m = (float)md;                                 // the shift: any value near the maximum, used exactly from here on
    float s = 0.f;
    for (int k = 0; k < NCE_JT; ++k) s = s + expf((float)(Ls[tid][k] - (double)m));
    vilco_st_agent(part + ((long)tid * nchunk + blockIdx.x) * 2, m);
    vilco_st_agent(part + ((long)tid * nchunk + blockIdx.x) * 2 + 1, s);
  }
}

// one workgroup of 2 * NCE_MAX_B threads: the log-sum-exp of every vector, then the loss
__global__ __launch_bounds__(2 * NCE_MAX_B) void ssl_nce_finish_kernel(const float* __restrict__ part, int nchunk,
                                                                      const float* __restrict__ mask, int B, float tau,
                                                                      float* __restrict__ stats, float* __restrict__ loss) {
  __shared__ float term[2 * NCE_MAX_B];
  const int v = threadIdx.x, V = 2 * B;
  if (v < V) {
    const float p = stats[2 * B + (v < B ? v : v - B)] / tau;
    const float* q = part + (long)v * nchunk * 2;
    float m = p;
    for (int k = 0; k < nchunk; ++k) m = fmaxf(m, vilco_ld_agent(q + 2 * k));
    float s = expf(p - m);
    for (int k = 0; k < nchunk; ++k) s = s + vilco_ld_agent(q + 2 * k + 1) * expf(vilco_ld_agent(q + 2 * k) - m);
    const float ls = logf(s);
    stats[3 * B + v] = m;
    stats[5 * B + v] = ls;
    term[v] = (m - p) + ls;
  }
  __syncthreads();
  if (v == 0) {
    double tot = 0.0;
    int n = 0;
    for (int b = 0; b < B; ++b)
      if (mask[b] != 0.f) { tot = tot + ((double)term[b] + (double)term[B + b]); ++n; }
    loss[0] = n > 0 ? (float)(tot / (2.0 * n)) : 0.f;
  }
}

// workgroup (column tile, slab of bank rows): part[slab][v][d] = sum_{j in slab} exp(logit_vj - lse_v) bank[j][d].
// Thread (tv = tid / 32, td = tid % 32) owns column td and the vectors tv + 8 a.
__global__ __launch_bounds__(ST) void ssl_nce_dxn_kernel(const double* __restrict__ logits, const float* __restrict__ stats,
                                                         const float* __restrict__ bank, int B, int D, int M, int tiles_per_slab,
                                                         float* __restrict__ part) {
  __shared__ float Bs[BW_JT][BW_DT + 1];
  __shared__ float Ps[2 * NCE_MAX_B][BW_JT + 1];
  const int tid = threadIdx.x, td = tid & 31, tv = tid >> 5, V = 2 * B;
  const int d0 = blockIdx.x * BW_DT, slab = blockIdx.y;
  const int jbeg = slab * tiles_per_slab * BW_JT;
  int jend = jbeg + tiles_per_slab * BW_JT;
  if (jend > M) jend = M;
  const float* shift = stats + 3 * B;
  const float* logs = stats + 5 * B;
  float acc[16];
#pragma unroll
  for (int a = 0; a < 16; ++a) acc[a] = 0.f;
  for (int j0 = jbeg; j0 < jend; j0 += BW_JT) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < BW_JT * BW_DT / ST; ++q) {
      const int idx = tid + q * ST, r = idx >> 5, c = idx & 31;
      const int j = j0 + r, d = d0 + c;
      Bs[r][c] = (j < jend && d < D) ? bank[(long)j * D + d] : 0.f;
    }
    for (int idx = tid; idx < V * BW_JT; idx += ST) {
      const int v = idx >> 5, jj = idx & 31, j = j0 + jj;
      Ps[v][jj] = j < jend ? expf((float)(logits[(long)v * M + j] - (double)shift[v]) - logs[v]) : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int jj = 0; jj < BW_JT; ++jj) {
      const float bv = Bs[jj][td];
#pragma unroll
      for (int a = 0; a < 16; ++a)
        if (tv + 8 * a < V) acc[a] = fmaf(Ps[tv + 8 * a][jj], bv, acc[a]);
    }
  }
  const int d = d0 + td;
  if (d < D) {
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int v = tv + 8 * a;
      if (v < V) vilco_st_agent(part + ((long)slab * V + v) * D + d, acc[a]);
    }
  }
}

// workgroup b: gradients of the raw text[b] and video[b]
__global__ __launch_bounds__(ST) void ssl_nce_bwd_finish_kernel(const float* __restrict__ gloss, const float* __restrict__ mask,
                                                                const float* __restrict__ xn, const float* __restrict__ stats,
                                                                const float* __restrict__ part, int nslab, int B, int D,
                                                                float tau, float* __restrict__ dtext, float* __restrict__ dvideo) {
  __shared__ float sd[ST];
  const int b = blockIdx.x, tid = threadIdx.x, V = 2 * B;
  float* gt = dtext + (long)b * D;
  float* gv = dvideo + (long)b * D;
  const int n = nce_count(mask, B);
  if (n == 0 || mask[b] == 0.f) {                               // uniform over the workgroup
    for (int d = tid; d < D; d += ST) { gt[d] = 0.f; gv[d] = 0.f; }
    return;
  }
  const float w = gloss[0] / (2.0f * (float)n);
  const float nt = stats[b], nv = stats[B + b], p = stats[2 * B + b] / tau;
  const float cpos = (expf((p - stats[3 * B + b]) - stats[5 * B + b]) + expf((p - stats[4 * B + b]) - stats[6 * B + b]) - 2.0f) / tau;
  const float* tn = xn + (long)b * D;
  const float* vn = xn + ((long)B + b) * D;
  float dt = 0.f, dv = 0.f;
  // first pass: the gradients of the normalised rows, kept in the outputs; their dot products with the rows
  for (int d = tid; d < D; d += ST) {
    float st = 0.f, sv = 0.f;
    for (int k = 0; k < nslab; ++k) {
      st = st + vilco_ld_agent(part + ((long)k * V + b) * D + d);
      sv = sv + vilco_ld_agent(part + ((long)k * V + B + b) * D + d);
    }
    const float a = w * (cpos * vn[d] + st / tau), c = w * (cpos * tn[d] + sv / tau);
    gt[d] = a; gv[d] = c;
    dt = dt + a * tn[d]; dv = dv + c * vn[d];
  }
  dt = block_sum(dt, sd);
  dv = block_sum(dv, sd);
  // x / max(||x||, eps): below eps the divisor is the constant
  const bool ct = nt <= 1e-12f, cv = nv <= 1e-12f;
  for (int d = tid; d < D; d += ST) {
    gt[d] = ct ? gt[d] / nt : (gt[d] - tn[d] * dt) / nt;
    gv[d] = cv ? gv[d] / nv : (gv[d] - vn[d] * dv) / nv;
  }
}

bool pool_plan(const int32_t* T, int32_t L, PoolDims* dm) {
  if (!T || L < 1 || L > SSL_MAX_L) return false;
  long s = 0;
  for (int l = 0; l < L; ++l) {
    if (T[l] < 1) return false;
    dm->T[l] = T[l];
    dm->soff[l] = (int)s;
    s += (T[l] + POOL_ROWS - 1) / POOL_ROWS;
  }
  for (int l = L; l <= SSL_MAX_L; ++l) {
    if (l < SSL_MAX_L) dm->T[l] = 0;
    dm->soff[l] = (int)s;
  }
  return s <= (1L << 24);
}

int nce_check(int32_t B, int32_t D, int32_t M) {
  if (B < 1 || D < 1 || M < 1 || (D % 4) != 0 || D > NCE_MAX_D || B > NCE_MAX_B || B > M) return VILCO_ERR_BADARG;
  return VILCO_OK;
}

int bw_slabs(int M, int* tiles_per_slab) {
  const int tiles = (M + BW_JT - 1) / BW_JT;
  int ns = tiles < BW_MAX_SLABS ? tiles : BW_MAX_SLABS;
  const int per = (tiles + ns - 1) / ns;
  ns = (tiles + per - 1) / per;
  *tiles_per_slab = per;
  return ns;
}

}  // namespace

extern "C" size_t vilco_ssl_pool_workspace(const int32_t* T, int32_t L, int32_t B, int32_t C) {
  PoolDims dm;
  if (B < 1 || C < 1 || !pool_plan(T, L, &dm)) return 0;
  return al256((size_t)B * dm.soff[L] * C * sizeof(float)) + 256;
}

extern "C" int vilco_ssl_pool_fwd(const float* const* feats, const int32_t* T, int32_t L, const int32_t* lens, int32_t B,
                                  int32_t C, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  PoolDims dm;
  if (L < 1 || L > SSL_MAX_L || B < 1 || B > 65535 || C < 1 || !feats || !lens || !out || !workspace) return VILCO_ERR_BADARG;
  if (!pool_plan(T, L, &dm)) return VILCO_ERR_BADARG;
  PoolSrc src;
  int vec = (C % 4) == 0;
  for (int l = 0; l < SSL_MAX_L; ++l) {
    src.p[l] = l < L ? feats[l] : nullptr;
    if (l < L && !feats[l]) return VILCO_ERR_BADARG;
    if (l < L && !vilco_aligned(feats[l], 16)) vec = 0;
  }
  if (workspace_bytes < vilco_ssl_pool_workspace(T, L, B, C)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  hipLaunchKernelGGL(ssl_pool_part_kernel, dim3(dm.soff[L], B), dim3(ST), 0, s, src, dm, (int)L, lens, (int)C, vec, part);
  hipLaunchKernelGGL(ssl_pool_finish_kernel, dim3((C + ST - 1) / ST, B), dim3(ST), 0, s, part, dm, (int)L, lens, (int)C, out);
  return vilco_launch_status();
}

extern "C" int vilco_ssl_pool_bwd(const float* dout, float* const* dfeats, const int32_t* T, int32_t L, const int32_t* lens,
                                  int32_t B, int32_t C, void* stream) {
  PoolDims dm;
  if (L < 1 || L > SSL_MAX_L || B < 1 || B > 65535 || C < 1 || !dout || !dfeats || !lens) return VILCO_ERR_BADARG;
  if (!pool_plan(T, L, &dm)) return VILCO_ERR_BADARG;
  PoolDst dst;
  int vec = (C % 4) == 0 && vilco_aligned(dout, 16);
  for (int l = 0; l < SSL_MAX_L; ++l) {
    dst.p[l] = l < L ? dfeats[l] : nullptr;
    if (l < L && !dfeats[l]) return VILCO_ERR_BADARG;
    if (l < L && !vilco_aligned(dfeats[l], 16)) vec = 0;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ssl_pool_bwd_kernel, dim3(dm.soff[L], B), dim3(ST), 0, s, dout, dst, dm, (int)L, lens, (int)C, vec);
  return vilco_launch_status();
}

extern "C" size_t vilco_ssl_nce_workspace(int32_t B, int32_t D, int32_t M) {
  if (nce_check(B, D, M) != VILCO_OK) return 0;
  int per;
  const size_t fwd = (size_t)2 * B * ((M + NCE_JT - 1) / NCE_JT) * 2 * sizeof(float);
  const size_t bwd = (size_t)bw_slabs(M, &per) * 2 * B * D * sizeof(float);
  return al256(fwd > bwd ? fwd : bwd) + 256;
}

extern "C" int vilco_ssl_ring_update(const float* rows, const float* mask, int32_t B, int32_t D, float* bank, int32_t M,
                                     int32_t* ring, void* stream) {
  const int rc = nce_check(B, D, M);
  if (rc != VILCO_OK) return rc;
  if (!rows || !mask || !bank || !ring || !vilco_aligned(rows, 16) || !vilco_aligned(bank, 16)) return VILCO_ERR_BADARG;
  hipLaunchKernelGGL(ssl_ring_kernel, dim3(1), dim3(RING_T), 0, reinterpret_cast<hipStream_t>(stream), rows, mask, (int)B,
                     (int)D, bank, (int)M, ring);
  return vilco_launch_status();
}

extern "C" int vilco_ssl_nce_fwd(const float* text, const float* video, const float* mask, int32_t B, int32_t D, float* bank,
                                 int32_t M, int32_t* ring, float temperature, float* xn, float* stats, double* logits,
                                 float* loss, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = nce_check(B, D, M);
  if (rc != VILCO_OK) return rc;
  if (!text || !video || !mask || !bank || !ring || !xn || !stats || !logits || !loss || !workspace) return VILCO_ERR_BADARG;
  if (!(temperature > 0.f) || !vilco_aligned(xn, 16) || !vilco_aligned(bank, 16)) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_ssl_nce_workspace(B, D, M)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const int nchunk = (M + NCE_JT - 1) / NCE_JT;
  hipLaunchKernelGGL(ssl_norm_kernel, dim3(B), dim3(ST), 0, s, text, video, (int)B, (int)D, xn, stats);
  hipLaunchKernelGGL(ssl_ring_kernel, dim3(1), dim3(RING_T), 0, s, xn, mask, (int)B, (int)D, bank, (int)M, ring);
  hipLaunchKernelGGL(ssl_logits_kernel, dim3(nchunk), dim3(ST), 0, s, xn, bank, 2 * (int)B, (int)D, (int)M, temperature, logits,
                     part);
  hipLaunchKernelGGL(ssl_nce_finish_kernel, dim3(1), dim3(2 * NCE_MAX_B), 0, s, part, nchunk, mask, (int)B, temperature, stats,
                     loss);
  return vilco_launch_status();
}

extern "C" int vilco_ssl_nce_bwd(const float* gloss, const float* mask, const float* xn, const float* stats, const double* logits,
                                 const float* bank, int32_t B, int32_t D, int32_t M, float temperature, float* dtext,
                                 float* dvideo, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = nce_check(B, D, M);
  if (rc != VILCO_OK) return rc;
  if (!gloss || !mask || !xn || !stats || !logits || !bank || !dtext || !dvideo || !workspace) return VILCO_ERR_BADARG;
  if (!(temperature > 0.f)) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_ssl_nce_workspace(B, D, M)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  int per;
  const int nslab = bw_slabs(M, &per);
  hipLaunchKernelGGL(ssl_nce_dxn_kernel, dim3((D + BW_DT - 1) / BW_DT, nslab), dim3(ST), 0, s, logits, stats, bank, (int)B, (int)D,
                     (int)M, per, part);
  hipLaunchKernelGGL(ssl_nce_bwd_finish_kernel, dim3(B), dim3(ST), 0, s, gloss, mask, xn, stats, part, nslab, (int)B, (int)D,
                     temperature, dtext, dvideo);
  return vilco_launch_status();
}
