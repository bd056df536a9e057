// Pooled Outputs Distillation (Douillard, Cord, Ollion, Robert, Valle: "PODNet: Pooled Outputs Distillation for Small-Tasks
// Incremental Learning", ECCV 2020; the reference has no feature-level distillation, so there is no line of it to cite) over
// the one-dimensional pyramid: every level's features [B][T_l][C] of a clip against the pooled, normalised record the
// incoming model's features of that clip left at the task boundary.
//
//   p[c] = sum_{t < V} fl(h[t][c]^2),  q[t] = sum_{c < C} fl(h[t][c]^2)       (squares fp32, sums fp64 in a fixed order)
//   v = [p ; q] (C + V entries),  n = max(||v||, 1e-12),  u = fl32(v / n)     (fp64, rounded to fp32 once: the value a
//                                                                              record holds, so that a clip against its own
//                                                                              record gives u - r = 0 exactly)
//   dist = ||u - r||,  out = (float)(scale / (L N_rec) sum_b sum_l dist),  0 when N_rec == 0           (fp64, one rounding)
//   g_v / w = ((u - r) / max(dist, 1e-12) - u (u . (u - r)) / max(dist, 1e-12)) / n                    (fp64, workspace)
//   d_h[t][c] = fl(fl(2 h) fl(gv[c] + gv[C + t])),  gv = fl32(w g_v / w),  w = g_out scale / (L N_rec) (fp64)
//
//   pod_tile_kernel     workgroup (time tile of TILE_T rows, batch row): a wave owns RPW rows; per 64 x VEC columns a lane
//                       keeps VEC column partials over its rows and one partial per row; the four waves' column partials
//                       are added through LDS in wave order and written as ONE partial per block and column, q[t] is
//                       finished by the wave's butterfly.  Rows without a record and tiles at or beyond V return at once.
//   pod_finish_kernel   workgroup (level, batch row): adds the block partials in block order, forms n, u, dist and leaves
//                       g_v / w where v was (or, for vilco_pod_record, writes u and zeros behind V into the record).
//   pod_sum_kernel      one workgroup: N_rec and the scalar.
//   pod_bwd_kernel      the tile grid again over ALL rows of every level: every element of every gradient is assigned --
//                       zeros at t >= V, for rows without a record and when N_rec == 0 (h is not read there).
// Three launches forward, two for a record, one backward, whatever B and L; no atomics: the same bits on every call.
// pod_tab and level_len are read when the kernels run.  Bytes: 4 per element forward, 8 backward (h, d_h).
#include "common.h"

namespace {

constexpr int PT = 256;                // threads per workgroup (4 waves)
constexpr int WPB = PT / 64;
constexpr int RPW = 8;                 // rows of a tile one wave owns
constexpr int TILE_T = WPB * RPW;      // rows of a tile
constexpr int POD_MAX_L = 16;
constexpr int FIN_B = 16;              // block partials the finish loads before it adds them

struct PodDims {
  int T[POD_MAX_L];
  int toff[POD_MAX_L + 1];             // first tile of every level, toff[L] = all tiles
  long eoff[POD_MAX_L + 1];            // first entry of every level's [p ; q] in a row's vector, eoff[L] = its width
};
struct PodSrc { const float* p[POD_MAX_L]; };
struct PodDst { float* p[POD_MAX_L]; };

struct PodWs {                         // the workspace, from its first 256-byte boundary
  int64_t* count;                      // N_rec
  double* dist;                        // [B][L]
  double* vec;                         // [B][eoff[L]]: v, then g_v / w
  double* part;                        // [B][toff[L]][C]: column partials per block
};

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

bool pod_plan(const int32_t* T, int L, int C, PodDims* dm) {
  if (!T || L < 1 || L > POD_MAX_L || C < 1) return false;
  long tiles = 0, e = 0;
  for (int l = 0; l < POD_MAX_L; ++l) {
    dm->T[l] = l < L ? T[l] : 0;
    dm->toff[l] = (int)tiles;
    dm->eoff[l] = e;
    if (l < L) {
      if (T[l] < 1) return false;
      tiles += (T[l] + TILE_T - 1) / TILE_T;
      e += (long)C + T[l];
      if (tiles > (1L << 30)) return false;
    }
  }
  dm->toff[POD_MAX_L] = (int)tiles;
  dm->eoff[POD_MAX_L] = e;
  for (int l = L; l < POD_MAX_L; ++l) { dm->toff[l] = (int)tiles; dm->eoff[l] = e; }
  return true;
}

size_t ws_bytes(const PodDims& dm, int B, int C, int L) {
  return 256 + al256(sizeof(int64_t)) + al256((size_t)B * L * sizeof(double)) +
         al256((size_t)B * dm.eoff[POD_MAX_L] * sizeof(double)) + al256((size_t)B * dm.toff[POD_MAX_L] * C * sizeof(double));
}

PodWs ws_view(void* workspace, const PodDims& dm, int B, int C, int L) {
  unsigned char* u = reinterpret_cast<unsigned char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  PodWs w;
  w.count = reinterpret_cast<int64_t*>(u); u += al256(sizeof(int64_t));
  w.dist = reinterpret_cast<double*>(u); u += al256((size_t)B * L * sizeof(double));
  w.vec = reinterpret_cast<double*>(u); u += al256((size_t)B * dm.eoff[POD_MAX_L] * sizeof(double));
  w.part = reinterpret_cast<double*>(u);
  return w;
}

__device__ __forceinline__ int pod_level(const PodDims& dm, int L, int tile) {
  int l = 0;
  while (l + 1 < L && tile >= dm.toff[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ int pod_len(const int* __restrict__ level_len, int b, int L, int l, int T) {
  const int n = level_len[b * L + l];
  return n < 0 ? 0 : (n > T ? T : n);
}

__device__ __forceinline__ double wave_sum_f64(double v) {     // fixed butterfly, result in every lane
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup in a fixed tree; the result in every thread.  `sd` has PT entries.
__device__ __forceinline__ double block_sum_f64(double v, double* sd) {
  const int tid = threadIdx.x;
  __syncthreads();                                             // sd may still be read from the previous call
  sd[tid] = v;
  __syncthreads();
  for (int o = PT / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  return sd[0];
}

template <int VEC>
__device__ __forceinline__ void load_row(const float* p, float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 a = *reinterpret_cast<const float4*>(p);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
  } else {
    x[0] = p[0];
  }
}

template <int VEC>
__device__ __forceinline__ void store_row(float* p, const float (&x)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
    p[0] = x[0];
  }
}

// pod_tab == nullptr: every row is pooled (vilco_pod_record)
template <int VEC>
__global__ __launch_bounds__(PT) void pod_tile_kernel(PodSrc src, PodDims dm, int L, int C, const int* __restrict__ level_len,
                                                      const int64_t* __restrict__ pod_tab, double* __restrict__ vec,
                                                      double* __restrict__ part) {
  __shared__ double sp[WPB][64 * VEC];
  const int b = blockIdx.y, tile = blockIdx.x;
  if (pod_tab && pod_tab[b] == 0) return;
  const int l = pod_level(dm, L, tile);
  const int T = dm.T[l];
  const int V = pod_len(level_len, b, L, l, T);
  const int t0 = (tile - dm.toff[l]) * TILE_T;
  if (t0 >= V) return;                                         // the finishing launch stops at the length too
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tw = t0 + wave * RPW;
  const float* f = src.p[l] + (long)b * T * C;
  double* pout = part + ((long)b * dm.toff[POD_MAX_L] + tile) * C;
  double qa[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) qa[r] = 0.0;
  for (int c0 = 0; c0 < C; c0 += 64 * VEC) {
    const int c = c0 + lane * VEC;
    float x[RPW][VEC];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) x[r][j] = 0.f;
      if (tw + r < V && c < C) load_row<VEC>(f + (long)(tw + r) * C + c, x[r]);
    }
    double pa[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) pa[j] = 0.0;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float s = x[r][j] * x[r][j];
        pa[j] = pa[j] + (double)s;
        qa[r] = qa[r] + (double)s;
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) sp[wave][lane * VEC + j] = pa[j];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * VEC; i += PT) {
      if (c0 + i < C) pout[c0 + i] = ((sp[0][i] + sp[1][i]) + sp[2][i]) + sp[3][i];
    }
    __syncthreads();
  }
  double* q = vec + (long)b * dm.eoff[POD_MAX_L] + dm.eoff[l] + C;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const double s = wave_sum_f64(qa[r]);
    if (lane == 0 && tw + r < V) q[tw + r] = s;
  }
}

// rec_out != nullptr: u goes to the records [B][eoff[L]] (zeros behind V) and nothing is compared
__global__ __launch_bounds__(PT) void pod_finish_kernel(PodDims dm, int L, int C, const int* __restrict__ level_len,
                                                        const int64_t* __restrict__ pod_tab, double* __restrict__ vec,
                                                        const double* __restrict__ part, double* __restrict__ dist,
                                                        float* __restrict__ rec_out) {
  __shared__ double sd[PT];
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int T = dm.T[l];
  const int V = pod_len(level_len, b, L, l, T);
  const long W = dm.eoff[POD_MAX_L];
  const int k = C + V;
  double* v = vec + (long)b * W + dm.eoff[l];
  float* ro = rec_out ? rec_out + (long)b * W + dm.eoff[l] : nullptr;
  const float* rec = nullptr;
  if (!rec_out) {
    const int64_t addr = pod_tab[b];
    if (addr != 0) rec = reinterpret_cast<const float*>(addr) + dm.eoff[l];
  }
  if ((!rec_out && !rec) || V == 0) {                          // block-uniform: nothing to compare / an empty level
    if (rec_out) {
      for (int i = tid; i < C + T; i += PT) ro[i] = 0.f;
    } else if (tid == 0) {
      dist[b * L + l] = 0.0;
    }
    return;
  }
  const int nt = (V + TILE_T - 1) / TILE_T;
  const double* p0 = part + ((long)b * dm.toff[POD_MAX_L] + dm.toff[l]) * C;
  double ss = 0.0;
  for (int i = tid; i < k; i += PT) {                          // thread tid owns the entries tid, tid + PT, ... throughout
    double s;
    if (i < C) {
      // block order, FIN_B loads in flight: a load per addition waits out one memory latency per block (72 of them at T = 2304,
      // 82 us); the loads past the last block repeat it and add an exact 0.0 instead
      s = 0.0;
      for (int j0 = 0; j0 < nt; j0 += FIN_B) {
        double x[FIN_B];
#pragma unroll
        for (int j = 0; j < FIN_B; ++j) {
          const int jj = j0 + j < nt ? j0 + j : nt - 1;
          x[j] = p0[(long)jj * C + i];
        }
#pragma unroll
        for (int j = 0; j < FIN_B; ++j) s = s + (j0 + j < nt ? x[j] : 0.0);
      }
      v[i] = s;
    } else {
      s = v[i];
    }
    ss = ss + s * s;
  }
  const double norm = sqrt(block_sum_f64(ss, sd));
  const double n = norm > 1e-12 ? norm : 1e-12;
  if (rec_out) {
    for (int i = tid; i < C + T; i += PT) ro[i] = i < k ? (float)(v[i] / n) : 0.f;
    return;
  }
  double dd = 0.0, ue = 0.0;
  for (int i = tid; i < k; i += PT) {
    const double u = (double)(float)(v[i] / n);
    const double e = u - (double)rec[i];
    dd = dd + e * e;
    ue = ue + u * e;
  }
  const double d = sqrt(block_sum_f64(dd, sd));
  const double dc = d > 1e-12 ? d : 1e-12;
  const double s = block_sum_f64(ue, sd) / dc;                 // u . g_u / w
  for (int i = tid; i < k; i += PT) {
    const double u = (double)(float)(v[i] / n);
    const double e = u - (double)rec[i];
    v[i] = (e / dc - u * s) / n;
  }
  if (tid == 0) dist[b * L + l] = d;
}

__global__ __launch_bounds__(PT) void pod_sum_kernel(int B, int L, const int64_t* __restrict__ pod_tab,
                                                     const double* __restrict__ dist, double scale, float* __restrict__ out,
                                                     int64_t* __restrict__ count) {
  __shared__ double sd[PT];
  const int tid = threadIdx.x;
  double n = 0.0, s = 0.0;                                     // (a count below 2^53: exact in a double)
  for (int b = tid; b < B; b += PT) n = n + (pod_tab[b] != 0 ? 1.0 : 0.0);
  for (long i = tid; i < (long)B * L; i += PT) s = s + dist[i];
  n = block_sum_f64(n, sd);
  s = block_sum_f64(s, sd);
  if (tid == 0) {
    count[0] = (int64_t)n;
    out[0] = n > 0.0 ? (float)(scale / ((double)L * n) * s) : 0.f;
  }
}

template <int VEC>
__global__ __launch_bounds__(PT) void pod_bwd_kernel(PodSrc src, PodDst dst, PodDims dm, int L, int C,
                                                     const int* __restrict__ level_len, const int64_t* __restrict__ pod_tab,
                                                     const double* __restrict__ vec, const int64_t* __restrict__ count,
                                                     const float* __restrict__ g_out, double scale) {
  const int b = blockIdx.y, tile = blockIdx.x;
  const int l = pod_level(dm, L, tile);
  const int T = dm.T[l];
  const int64_t N = count[0];
  const int V = (N > 0 && pod_tab[b] != 0) ? pod_len(level_len, b, L, l, T) : 0;
  const int t0 = (tile - dm.toff[l]) * TILE_T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tw = t0 + wave * RPW;
  const float* f = src.p[l] + (long)b * T * C;
  float* d = dst.p[l] + (long)b * T * C;
  const double* gv = vec + (long)b * dm.eoff[POD_MAX_L] + dm.eoff[l];
  const double w = N > 0 ? (double)g_out[0] * scale / ((double)L * (double)N) : 0.0;
  float gt[RPW];
#pragma unroll
  for (int r = 0; r < RPW; ++r) gt[r] = tw + r < V ? (float)(w * gv[C + tw + r]) : 0.f;
  for (int c0 = 0; c0 < C; c0 += 64 * VEC) {
    const int c = c0 + lane * VEC;
    if (c >= C) continue;
    float gc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) gc[j] = tw < V ? (float)(w * gv[c + j]) : 0.f;
    float x[RPW][VEC];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) x[r][j] = 0.f;
      if (tw + r < V) load_row<VEC>(f + (long)(tw + r) * C + c, x[r]);
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      if (tw + r >= T) break;
      float o[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] = tw + r < V ? (2.f * x[r][j]) * (gc[j] + gt[r]) : 0.f;
      store_row<VEC>(d + (long)(tw + r) * C + c, o);
    }
  }
}

// everything a launch relies on, checked on the host
int check_desc(const vilco_pod_desc* d, bool need_tab, PodDims* dm, PodSrc* src, int* vec) {
  if (!d || !d->feats || !d->level_T || !d->level_len || (need_tab && !d->pod_tab)) return VILCO_ERR_BADARG;
  if (d->L < 1 || d->L > POD_MAX_L || d->B < 1 || d->B > 65535 || d->C < 1) return VILCO_ERR_BADARG;
  if (!pod_plan(d->level_T, d->L, d->C, dm)) return VILCO_ERR_BADARG;
  *vec = (d->C % 4) == 0;
  for (int l = 0; l < POD_MAX_L; ++l) {
    src->p[l] = l < d->L ? d->feats[l] : nullptr;
    if (l < d->L && !d->feats[l]) return VILCO_ERR_BADARG;
    if (l < d->L && !vilco_aligned(d->feats[l], 16)) *vec = 0;
  }
  return VILCO_OK;
}

void launch_tiles(const vilco_pod_desc* d, const PodDims& dm, const PodSrc& src, int vec, const int64_t* tab, const PodWs& w,
                  hipStream_t s) {
  const dim3 grid(dm.toff[POD_MAX_L], d->B);
  if (vec)
    hipLaunchKernelGGL(pod_tile_kernel<4>, grid, dim3(PT), 0, s, src, dm, (int)d->L, (int)d->C, d->level_len, tab, w.vec, w.part);
  else
    hipLaunchKernelGGL(pod_tile_kernel<1>, grid, dim3(PT), 0, s, src, dm, (int)d->L, (int)d->C, d->level_len, tab, w.vec, w.part);
}

}  // namespace

extern "C" int32_t vilco_pod_tile_rows(void) { return TILE_T; }

extern "C" size_t vilco_pod_workspace(const int32_t* level_T, int32_t L, int32_t B, int32_t C) {
  PodDims dm;
  if (B < 1 || !pod_plan(level_T, L, C, &dm)) return 0;
  return ws_bytes(dm, B, C, L);
}

extern "C" int vilco_pod_fwd(const vilco_pod_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  PodDims dm;
  PodSrc src;
  int vec = 0;
  const int rc = check_desc(d, true, &dm, &src, &vec);
  if (rc != VILCO_OK) return rc;
  if (!out || !workspace) return VILCO_ERR_BADARG;
  if (workspace_bytes < ws_bytes(dm, d->B, d->C, d->L)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const PodWs w = ws_view(workspace, dm, d->B, d->C, d->L);
  launch_tiles(d, dm, src, vec, d->pod_tab, w, s);
  hipLaunchKernelGGL(pod_finish_kernel, dim3(d->L, d->B), dim3(PT), 0, s, dm, (int)d->L, (int)d->C, d->level_len, d->pod_tab,
                     w.vec, (const double*)w.part, w.dist, (float*)nullptr);
  hipLaunchKernelGGL(pod_sum_kernel, dim3(1), dim3(PT), 0, s, (int)d->B, (int)d->L, d->pod_tab, (const double*)w.dist, d->scale,
                     out, w.count);
  return vilco_launch_status();
}

extern "C" int vilco_pod_record(const vilco_pod_desc* d, float* records, void* workspace, size_t workspace_bytes, void* stream) {
  PodDims dm;
  PodSrc src;
  int vec = 0;
  const int rc = check_desc(d, false, &dm, &src, &vec);
  if (rc != VILCO_OK) return rc;
  if (!records || !workspace) return VILCO_ERR_BADARG;
  if (workspace_bytes < ws_bytes(dm, d->B, d->C, d->L)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const PodWs w = ws_view(workspace, dm, d->B, d->C, d->L);
  launch_tiles(d, dm, src, vec, nullptr, w, s);
  hipLaunchKernelGGL(pod_finish_kernel, dim3(d->L, d->B), dim3(PT), 0, s, dm, (int)d->L, (int)d->C, d->level_len,
                     (const int64_t*)nullptr, w.vec, (const double*)w.part, w.dist, records);
  return vilco_launch_status();
}

extern "C" int vilco_pod_bwd(const vilco_pod_desc* d, const float* g_out, float* const* d_feats, const void* workspace,
                             size_t workspace_bytes, void* stream) {
  PodDims dm;
  PodSrc src;
  int vec = 0;
  const int rc = check_desc(d, true, &dm, &src, &vec);
  if (rc != VILCO_OK) return rc;
  if (!g_out || !d_feats || !workspace) return VILCO_ERR_BADARG;
  PodDst dst;
  for (int l = 0; l < POD_MAX_L; ++l) {
    dst.p[l] = l < d->L ? d_feats[l] : nullptr;
    if (l < d->L && !d_feats[l]) return VILCO_ERR_BADARG;
    if (l < d->L && !vilco_aligned(d_feats[l], 16)) vec = 0;
  }
  if (workspace_bytes < ws_bytes(dm, d->B, d->C, d->L)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const PodWs w = ws_view(const_cast<void*>(workspace), dm, d->B, d->C, d->L);
  const dim3 grid(dm.toff[POD_MAX_L], d->B);
  if (vec)
    hipLaunchKernelGGL(pod_bwd_kernel<4>, grid, dim3(PT), 0, s, src, dst, dm, (int)d->L, (int)d->C, d->level_len, d->pod_tab,
                       (const double*)w.vec, (const int64_t*)w.count, g_out, d->scale);
  else
    hipLaunchKernelGGL(pod_bwd_kernel<1>, grid, dim3(PT), 0, s, src, dst, dm, (int)d->L, (int)d->C, d->level_len, d->pod_tab,
                       (const double*)w.vec, (const int64_t*)w.count, g_out, d->scale);
  return vilco_launch_status();
}
