// Herding exemplar selection for the replay memory (iCaRL's prioritised exemplar list; the reference's own branch,
// MQ/libs/modeling/meta_archs.py:973-1043, is commented out and unfinished).  A clip's descriptor is its whole feature
// pyramid, one map per level divided by its Frobenius norm; everything the greedy selection needs follows from the per-level
// Gram matrices G = Phi Phi^T of the N candidates of a class (include/vilco_hip.h has the identities).
//
//   vilco_frob_scale   inverse Frobenius norm of every row of X[N, D]: per (row, segment) workgroup a fixed tree over
//                      per-thread fp32 sums (the tree itself in fp64), then one thread per row adds the segments in order.
//   vilco_gram         G = X X^T, fp32 in, exact fp32 products on v_mfma_f32_32x32x2_f32, fp32 accumulation.  Split-K over
//                      the whole chip: workgroup (slab, I, J) owns a K slab and the 32x32 tiles of the 96-row super blocks
//                      I >= J; it stages [rows][64] chunks of X through LDS (next chunk's global loads in flight while the
//                      MFMAs run), every wave takes a quarter of the chunk's k range over ALL tiles (balanced whatever the
//                      tile count), the four waves' accumulators are added through LDS in wave order and written as the
//                      slab's partial.  A second launch adds the partials in slab order in fp64, applies the optional row
//                      scales and mirrors the lower triangle, so G is exactly symmetric.  With N <= 96 every element of X
//                      is read from HBM once.
//   vilco_herd_select  one workgroup per class, fp64, this file is compiled with -ffp-contract=off: row sums, then
//                      min(m, N) greedy steps of O(N L) work each over the running r_i = sum_{j in sel} G_ij,
//                      s = sum_{j,j' in sel} G_jj' and t = sum_{j in sel} a_j; argmin by a fixed tree, lowest index on ties.
// No float atomics, no allocation, no host synchronisation; repeated calls are bit-equal.
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

namespace {

constexpr int GT = 256;                // threads per workgroup (4 waves)
constexpr int KC = 64;                 // k values per staged chunk: 16 per wave
constexpr int LDK = KC + 4;            // LDS row stride in floats: 16-byte aligned rows, b128 row reads conflict-free
constexpr int SB = 3;                  // 32-row blocks per super block
constexpr int SBR = SB * 32;           // rows per super block
constexpr int GRAM_TARGET_WGS = 1024;  // ~4 workgroups per CU
constexpr int HS_MAX_L = 16;
constexpr int HS_MAX_N = 4096;
constexpr int FR_SEG = 16384;          // elements per frob segment (64 per thread)
constexpr int FR_MAX_SEG = 256;

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------------------- frob scale
__global__ __launch_bounds__(GT) void frob_part_kernel(const float* __restrict__ x, long ld, long D, long seglen, int vec,
                                                       double* __restrict__ part, int nseg) {
  __shared__ double sd[GT];
  const int row = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  const float* p = x + (long)row * ld;
  const long k0 = (long)seg * seglen;
  const long k1 = k0 + seglen < D ? k0 + seglen : D;
  float acc = 0.f;
  if (vec) {                                                   // seglen % 4 == 0, rows 16-byte aligned
    long k = k0 + (long)tid * 4;
    for (; k + 4 <= k1; k += GT * 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + k);
      acc = acc + v.x * v.x; acc = acc + v.y * v.y; acc = acc + v.z * v.z; acc = acc + v.w * v.w;
    }
    if (k < k1)                                                // the row's last, short quad
      for (long e = k; e < k1; ++e) acc = acc + p[e] * p[e];
  } else {
    for (long k = k0 + tid; k < k1; k += GT) acc = acc + p[k] * p[k];
  }
  sd[tid] = (double)acc;
  __syncthreads();
  for (int o = GT / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  if (tid == 0) part[(long)row * nseg + seg] = sd[0];
}

__global__ __launch_bounds__(GT) void frob_finish_kernel(const double* __restrict__ part, int nseg, int rows,
                                                         float* __restrict__ inv) {
  const int row = blockIdx.x * GT + threadIdx.x;
  if (row >= rows) return;
  double s = 0.0;
  for (int g = 0; g < nseg; ++g) s = s + part[(long)row * nseg + g];
  inv[row] = (float)(1.0 / sqrt(s));
}

// ---------------------------------------------------------------------------------------------------------------- gram
struct GramPlan {
  int nsb;            // super blocks
  int nchunk;         // 64-wide chunks of D
  int cps;            // chunks per slab
  int nslab;
  size_t bytes;       // partials: [nslab][N][N] floats
};

GramPlan gram_plan(long N, long D) {
  GramPlan p;
  p.nsb = (int)((N + SBR - 1) / SBR);
  const long nst = (long)p.nsb * (p.nsb + 1) / 2;
  const long nchunk = (D + KC - 1) / KC;
  long target = GRAM_TARGET_WGS / nst;
  if (target < 1) target = 1;
  long nslab = nchunk < target ? nchunk : target;
  if (nslab < 1) nslab = 1;
  const long cps = (nchunk + nslab - 1) / nslab;
  p.nchunk = (int)nchunk;
  p.cps = (int)(cps < 1 ? 1 : cps);
  p.nslab = (int)((nchunk + p.cps - 1) / p.cps);
  if (p.nslab < 1) p.nslab = 1;
  p.bytes = al256((size_t)p.nslab * N * N * sizeof(float));
  return p;
}

// four values of one staged row; everything outside [0, N) x [0, D) is zero
__device__ __forceinline__ float4 gram_load(const float* __restrict__ x, long ld, int N, long D, int vec, int grow, long k) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (grow < N && k < D) {
    const float* p = x + (long)grow * ld + k;                 // 64-bit row offset: N * D may pass 2^31 elements
    if (vec && k + 4 <= D) {
      v = *reinterpret_cast<const float4*>(p);
    } else {
      v.x = p[0];
      if (k + 1 < D) v.y = p[1];
      if (k + 2 < D) v.z = p[2];
      if (k + 3 < D) v.w = p[3];
    }
  }
  return v;
}

// DIAG: super tile (I, I), one super block staged, the lower triangle of its tiles (96 accumulator registers: two waves per
// SIMD); otherwise super tile (I, J < I), two super blocks staged, all nine tiles
template <bool DIAG>
__global__ __launch_bounds__(GT) void gram_kernel(const float* __restrict__ x, long ld, int N, long D, int vec, int cps,
                                                  int nchunk, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float lds[(DIAG ? 1 : 2) * SBR * LDK];
  const int I = blockIdx.y, J = DIAG ? blockIdx.y : blockIdx.z;
  if (!DIAG && J >= I) return;
  constexpr bool diag = DIAG;
  constexpr int NQ = (DIAG ? 1 : 2) * SBR * (KC / 4) / GT;     // float4 items per thread and chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.x;
  const int c0 = slab * cps, c1 = (c0 + cps < nchunk) ? c0 + cps : nchunk;
  // 32-row blocks of each super block that hold a row at all (wave-uniform)
  const int nbI = (((N - I * SBR) < SBR ? (N - I * SBR) : SBR) + 31) / 32;
  const int nbJ = (((N - J * SBR) < SBR ? (N - J * SBR) : SBR) + 31) / 32;

  f32x16 acc[SB][SB];
#pragma unroll
  for (int a = 0; a < SB; ++a)
#pragma unroll
    for (int b = 0; b < SB; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;

  // item (row, c4) of a chunk: 16 consecutive lanes read one row's 256 contiguous bytes
  float4 pre[NQ];
  auto fetch = [&](int c) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      {
        const int idx = tid + q * GT;
        const int srow = idx >> 4, c4 = idx & 15;
        const int grow = srow < SBR ? I * SBR + srow : J * SBR + (srow - SBR);
        pre[q] = gram_load(x, ld, N, D, vec, grow, (long)c * KC + c4 * 4);
      }
    }
  };
  if (c0 < c1) fetch(c0);
  for (int c = c0; c < c1; ++c) {
    __syncthreads();                                           // the previous chunk has been consumed
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      {
        const int idx = tid + q * GT;
        *reinterpret_cast<float4*>(&lds[(idx >> 4) * LDK + (idx & 15) * 4]) = pre[q];
      }
    }
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);                              // in flight while the MFMAs below run
    // lanes 0-31 hold k = koff .. koff+3 of their row, lanes 32-63 the next four: four 32x32x2 steps cover eight k values
    // (the order of k inside a sum is free as long as both operands use the same one)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int koff = wave * 16 + h * 8 + (lane >> 5) * 4;
      float4 xa[SB], xb[SB];
#pragma unroll
      for (int a = 0; a < SB; ++a) {
        xa[a] = *reinterpret_cast<const float4*>(&lds[(a * 32 + (lane & 31)) * LDK + koff]);
        xb[a] = xa[a];
      }
      if (!diag) {
#pragma unroll
        for (int b = 0; b < SB; ++b) xb[b] = *reinterpret_cast<const float4*>(&lds[(SBR + b * 32 + (lane & 31)) * LDK + koff]);
      }
#pragma unroll
      for (int a = 0; a < SB; ++a) {
#pragma unroll
        for (int b = 0; b < SB; ++b) {
          if (a < nbI && b < nbJ && (!diag || b <= a)) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[a].x, xb[b].x, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[a].y, xb[b].y, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[a].z, xb[b].z, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[a].w, xb[b].w, acc[a][b], 0, 0, 0);
          }
        }
      }
    }
  }
  // the four waves' accumulators, tile by tile, added in wave order; C/D map of the 32x32 forms: column = lane & 31,
  // row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* pout = part + (long)slab * N * N;
#pragma unroll
  for (int a = 0; a < SB; ++a) {
#pragma unroll
    for (int b = 0; b < SB; ++b) {
      if (a < nbI && b < nbJ && (!diag || b <= a)) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) lds[wave * 1024 + r * 64 + lane] = acc[a][b][r];
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = tid + e * GT;
          const int r = idx >> 6, l = idx & 63;
          const float v = (lds[idx] + lds[1024 + idx]) + (lds[2048 + idx] + lds[3072 + idx]);
          const int gi = I * SBR + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
          const int gj = J * SBR + b * 32 + (l & 31);
          if (gi < N && gj < N) pout[(long)gi * N + gj] = v;
        }
      }
    }
  }
}

// G[i][j] = scale_i scale_j sum_slab part[slab][hi][lo], hi = max(i, j), lo = min(i, j): the tile that holds (hi, lo) was
// written by every slab; the other triangle is its mirror
template <typename OUT>
__global__ __launch_bounds__(GT) void gram_finish_kernel(const float* __restrict__ part, int nslab, int N,
                                                         const float* __restrict__ scale, OUT* __restrict__ g) {
  const long e = (long)blockIdx.x * GT + threadIdx.x;
  const long nn = (long)N * N;
  if (e >= nn) return;
  const int i = (int)(e / N), j = (int)(e % N);
  const int hi = i > j ? i : j, lo = i > j ? j : i;
  const float* p = part + (long)hi * N + lo;
  double s = 0.0;
  for (int k = 0; k < nslab; ++k) s = s + (double)p[(long)k * nn];
  if (scale) s = s * ((double)scale[hi] * (double)scale[lo]);
  g[e] = (OUT)s;
}

// -------------------------------------------------------------------------------------------------------------- select
__device__ __forceinline__ bool hs_better(double c1, int i1, double c2, int i2) {
  return c1 < c2 || (c1 == c2 && i1 < i2);
}

// one workgroup per class.  g: [cls][L][N][N] fp64; ws: [cls][2][L][N] fp64 (a, r); sel: [cls][min(m, N)]
__global__ __launch_bounds__(GT) void herd_select_kernel(const double* __restrict__ g_, int L, int N, int npick,
                                                         double* __restrict__ ws_, int* __restrict__ sel_) {
  __shared__ unsigned char taken[HS_MAX_N];
  __shared__ double s_[HS_MAX_L], t_[HS_MAX_L], tot_[HS_MAX_L];
  __shared__ double bc[GT];
  __shared__ int bi[GT];
  __shared__ int pick;
  const int tid = threadIdx.x;
  const long nn = (long)N * N;
  const double* g = g_ + (long)blockIdx.x * L * nn;
  double* a_ = ws_ + (long)blockIdx.x * 2 * L * N;
  double* r_ = a_ + (long)L * N;
  int* sel = sel_ + (long)blockIdx.x * npick;
  // row sums, each in index order
  for (int i = tid; i < N; i += GT) {
    taken[i] = 0;
    for (int l = 0; l < L; ++l) {
      const double* row = g + l * nn + (long)i * N;
      double s = 0.0;
      for (int j = 0; j < N; ++j) s = s + row[j];
      a_[(long)l * N + i] = s;
      r_[(long)l * N + i] = 0.0;
    }
  }
  __syncthreads();
  if (tid < L) {                                               // sum(G) = the row sums added in index order
    double s = 0.0;
    for (int i = 0; i < N; ++i) s = s + a_[(long)tid * N + i];
    tot_[tid] = sqrt(s);
    s_[tid] = 0.0;
    t_[tid] = 0.0;
  }
  __syncthreads();
  for (int i = tid; i < N; i += GT)
    for (int l = 0; l < L; ++l) a_[(long)l * N + i] = a_[(long)l * N + i] / tot_[l];          // a_i = mu . phi_i
  __syncthreads();
  for (int step = 0; step < npick; ++step) {
    double best = __longlong_as_double(0x7ff0000000000000ll);
    int besti = 0x7fffffff;
    for (int i = tid; i < N; i += GT) {
      if (taken[i]) continue;
      double cost = 0.0;
      for (int l = 0; l < L; ++l) {
        const double d = g[l * nn + (long)i * N + i];
        const double num = 2.0 * (a_[(long)l * N + i] + t_[l]);
        const double den = sqrt((d + 2.0 * r_[(long)l * N + i]) + s_[l]);
        cost = cost + (2.0 - num / den);
      }
      if (cost != cost) cost = __longlong_as_double(0x7ff0000000000000ll);     // NaN ranks with +inf
      if (hs_better(cost, i, best, besti)) { best = cost; besti = i; }
    }
    bc[tid] = best;
    bi[tid] = besti;
    __syncthreads();
    for (int o = GT / 2; o >= 1; o >>= 1) {
      if (tid < o && hs_better(bc[tid + o], bi[tid + o], bc[tid], bi[tid])) { bc[tid] = bc[tid + o]; bi[tid] = bi[tid + o]; }
      __syncthreads();
    }
    if (tid == 0) { pick = bi[0]; sel[step] = bi[0]; taken[bi[0]] = 1; }
    __syncthreads();
    const int p = pick;
    if (tid < L) {                                             // with r before this step's update
      s_[tid] = (s_[tid] + 2.0 * r_[(long)tid * N + p]) + g[tid * nn + (long)p * N + p];
      t_[tid] = t_[tid] + a_[(long)tid * N + p];
    }
    __syncthreads();
    for (int i = tid; i < N; i += GT)
      for (int l = 0; l < L; ++l) r_[(long)l * N + i] = r_[(long)l * N + i] + g[l * nn + (long)p * N + i];
    __syncthreads();
  }
}

int frob_nseg(long D) {
  long n = (D + FR_SEG - 1) / FR_SEG;
  return (int)(n < 1 ? 1 : (n > FR_MAX_SEG ? FR_MAX_SEG : n));
}

}  // namespace

extern "C" size_t vilco_frob_scale_workspace(int64_t rows, int64_t D) {
  if (rows < 0 || D < 0) return 0;
  return al256((size_t)(rows > 0 ? rows : 1) * frob_nseg(D) * sizeof(double)) + 256;
}

extern "C" int vilco_frob_scale(const float* x, int64_t rows, int64_t D, int64_t ld, float* inv_norm, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (rows < 0 || D < 0 || ld < D) return VILCO_ERR_BADARG;
  if (rows > 0 && (!x || !inv_norm || !workspace)) return VILCO_ERR_BADARG;
  if (rows > 65535) return VILCO_ERR_UNSUPPORTED;
  if (workspace_bytes < vilco_frob_scale_workspace(rows, D)) return VILCO_ERR_WORKSPACE;
  if (rows == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const int nseg = frob_nseg(D);
  long seglen = (D + nseg - 1) / nseg;
  seglen = (seglen + 3) / 4 * 4;
  if (seglen < 4) seglen = 4;
  const int vec = vilco_aligned(x, 16) && (ld % 4) == 0;
  hipLaunchKernelGGL(frob_part_kernel, dim3(nseg, (unsigned)rows), dim3(GT), 0, s, x, (long)ld, (long)D, seglen, vec, part, nseg);
  hipLaunchKernelGGL(frob_finish_kernel, dim3((unsigned)((rows + GT - 1) / GT)), dim3(GT), 0, s, part, nseg, (int)rows, inv_norm);
  return vilco_launch_status();
}

extern "C" size_t vilco_gram_workspace(int64_t N, int64_t D) {
  if (N < 0 || D < 0 || N > 32767) return 0;
  return gram_plan(N > 0 ? N : 1, D).bytes + 256;
}

extern "C" int vilco_gram(const float* x, int64_t N, int64_t D, int64_t ld, const float* row_scale, void* g, int32_t g_fp64,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 0 || D < 0 || ld < D) return VILCO_ERR_BADARG;
  if (N > 0 && (!g || !workspace || (D > 0 && !x))) return VILCO_ERR_BADARG;
  if (N > 32767) return VILCO_ERR_UNSUPPORTED;
  if (workspace_bytes < vilco_gram_workspace(N, D)) return VILCO_ERR_WORKSPACE;
  if (N == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const GramPlan p = gram_plan(N, D);
  const int vec = vilco_aligned(x, 16) && (ld % 4) == 0;
  // D == 0: one slab of zero chunks writes zero partials
  hipLaunchKernelGGL(gram_kernel<true>, dim3(p.nslab, p.nsb, 1), dim3(GT), 0, s, x, (long)ld, (int)N, (long)D, vec, p.cps,
                     p.nchunk, part);
  if (p.nsb > 1)
    hipLaunchKernelGGL(gram_kernel<false>, dim3(p.nslab, p.nsb, p.nsb), dim3(GT), 0, s, x, (long)ld, (int)N, (long)D, vec, p.cps,
                       p.nchunk, part);
  const unsigned nb = (unsigned)(((long)N * N + GT - 1) / GT);
  if (g_fp64)
    hipLaunchKernelGGL(gram_finish_kernel<double>, dim3(nb), dim3(GT), 0, s, part, p.nslab, (int)N, row_scale,
                       reinterpret_cast<double*>(g));
  else
    hipLaunchKernelGGL(gram_finish_kernel<float>, dim3(nb), dim3(GT), 0, s, part, p.nslab, (int)N, row_scale,
                       reinterpret_cast<float*>(g));
  return vilco_launch_status();
}

extern "C" size_t vilco_herd_select_workspace(int32_t n_cls, int32_t L, int32_t N) {
  if (n_cls < 0 || L < 0 || N < 0) return 0;
  return al256((size_t)(n_cls > 0 ? n_cls : 1) * 2 * (L > 0 ? L : 1) * (N > 0 ? N : 1) * sizeof(double)) + 256;
}

extern "C" int vilco_herd_select(const double* grams, int32_t n_cls, int32_t L, int32_t N, int32_t m, int32_t* sel,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (n_cls < 0 || L < 0 || N < 0 || m < 0) return VILCO_ERR_BADARG;
  const int npick = m < N ? m : N;
  if (n_cls > 0 && npick > 0 && (!grams || !sel || !workspace)) return VILCO_ERR_BADARG;
  if (L < 1 || L > HS_MAX_L || N > HS_MAX_N) return VILCO_ERR_UNSUPPORTED;
  if (workspace_bytes < vilco_herd_select_workspace(n_cls, L, N)) return VILCO_ERR_WORKSPACE;
  if (n_cls == 0 || npick == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  double* ws = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  hipLaunchKernelGGL(herd_select_kernel, dim3(n_cls), dim3(GT), 0, s, grams, (int)L, (int)N, npick, ws, sel);
  return vilco_launch_status();
}
