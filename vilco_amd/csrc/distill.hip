// Distillation term of iCaRL / BiC (MQ/libs/modeling/meta_archs.py:1482-1519) and its gradient, one call each way.
// From the second task on the reference adds, per pyramid level l (T_l rows; padded positions count, :1493 / :1513):
//
//   mode 0, iCaRL (:1501-1519)   0.01 * (1/T_l) sum_t sum_{y < n_known} bce(x[clip, t, y], p_l[t, y])
//                                bce(x, p) = max(x, 0) - x p + log1p(exp(-|x|))          (nn.BCEWithLogitsLoss per class y)
//   mode 1, BiC, T = 2 (:1482-1499)   scale * -(1/T_l) sum_t sum_{y < n_known} p_l[t, y] log_softmax(x[clip, t, :n_known] / 2)[y]
//
// x = the concatenated head output [B][R][C] the label / loss kernels read (levels end to end, separator rows allowed:
// level l occupies rows level_row[l] .. level_row[l] + level_T[l]); p = the cached outputs of the previous model,
// [sum T_l][ldt], levels end to end without separators.  Only batch row `clip` enters (the reference: row 0).
//
//   distill_fwd_kernel     one wavefront per row (a block's four waves walk rows w, w + 4 gridDim.x, ...): lanes stride over
//                          the n_known classes, the BiC row maximum and sums are wave reductions; a wave adds its rows'
//                          values / T_l in fp64 in row order, the four waves are added in order: one partial per block.
//   distill_finish_kernel  one workgroup adds the partials in block order (fixed tree) and writes the fp32 loss.
//   distill_bwd_kernel     one wavefront per row again; every element of d_logits[clip, level rows, :n_known] has one
//                          owner lane.  iCaRL: g 0.01/T_l (sigmoid(x) - p); BiC: g scale/T_l 1/2 (softmax(x/2)[y] sum_y p - p[y])
//                          (sum_y p is formed, not assumed 1).  g is read from device memory.  Nothing else of d_logits is
//                          written: other clips, separator rows and columns >= n_known belong to the caller.
// Two launches forward, one backward, whatever n_known and L; no atomics: the same bits on every call.
#include "common.h"

namespace {

constexpr int DT = 256;                // threads per workgroup (4 waves)
constexpr int WPB = DT / 64;
constexpr int MAX_BLOCKS = 1024;

struct DistillArgs {
  const float* logits;
  const float* targets;
  const int32_t* level_dev;            // [2][L]: first rows, lengths (the device copy of the validated host arrays)
  long N;                              // sum of level_T
  int R, C, L, clip, ldt, n_known, mode;
  float coef;                          // 0.01 (iCaRL) or scale (BiC)
};

int grid_blocks(long N) {
  const long g = (N + WPB - 1) / WPB;
  return (int)(g < 1 ? 1 : (g > MAX_BLOCKS ? MAX_BLOCKS : g));
}

// row n of the target buffer -> its row of the logits and 1/T of its level; false: the device table disagrees with the
// validated bounds (nothing is read or written for such a row)
__device__ __forceinline__ bool locate(const DistillArgs& a, long n, long* xrow, float* inv_T) {
  long first = 0;
  for (int l = 0; l < a.L; ++l) {
    const int T = a.level_dev[a.L + l];
    if (T <= 0) return false;
    if (n < first + T) {
      const long r = (long)a.level_dev[l] + (n - first);
      if (a.level_dev[l] < 0 || r >= a.R) return false;
      *xrow = r;
      *inv_T = 1.f / (float)T;
      return true;
    }
    first += T;
  }
  return false;
}

__device__ __forceinline__ float bce_logits(float x, float p) {
  return fmaxf(x, 0.f) - x * p + log1pf(expf(-fabsf(x)));
}

// max_y x[y] / 2 and sum_y exp(x[y] / 2 - max) of one row, in every lane
__device__ __forceinline__ void softmax_stats(const float* __restrict__ x, int n_known, int lane, float* mx, float* se) {
  float m = -INFINITY;
  for (int y = lane; y < n_known; y += 64) m = fmaxf(m, 0.5f * x[y]);
  m = wave_max(m);
  float s = 0.f;
  for (int y = lane; y < n_known; y += 64) s += expf(0.5f * x[y] - m);
  *mx = m;
  *se = wave_sum(s);
}

__global__ __launch_bounds__(DT) void distill_fwd_kernel(DistillArgs a, double* __restrict__ part) {
  __shared__ double sw[WPB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (long n = (long)blockIdx.x * WPB + wave; n < a.N; n += (long)gridDim.x * WPB) {      // wave-uniform
    long xrow;
    float inv_T;
    if (!locate(a, n, &xrow, &inv_T)) continue;
    const float* x = a.logits + ((long)a.clip * a.R + xrow) * a.C;
    const float* p = a.targets + n * a.ldt;
    float v = 0.f;
    if (a.mode == 0) {
      for (int y = lane; y < a.n_known; y += 64) v += bce_logits(x[y], p[y]);
    } else {
      float m, s;
      softmax_stats(x, a.n_known, lane, &m, &s);
      const float lse = m + logf(s);
      for (int y = lane; y < a.n_known; y += 64) v += p[y] * (lse - 0.5f * x[y]);          // -p log_softmax: terms >= 0 for p >= 0
    }
    acc = acc + (double)(wave_sum(v) * inv_T);
  }
  if (lane == 0) sw[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = sw[0];
    for (int k = 1; k < WPB; ++k) v = v + sw[k];
    part[blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(DT) void distill_finish_kernel(const double* __restrict__ part, int nblk, float coef,
                                                            float* __restrict__ out) {
  __shared__ double sd[DT];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int b = tid; b < nblk; b += DT) v = v + part[b];
  sd[tid] = v;
  __syncthreads();
  for (int o = DT / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)((double)coef * sd[0]);
}

__global__ __launch_bounds__(DT) void distill_bwd_kernel(DistillArgs a, const float* __restrict__ g_out,
                                                         float* __restrict__ d_logits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float g = g_out[0] * a.coef;
  for (long n = (long)blockIdx.x * WPB + wave; n < a.N; n += (long)gridDim.x * WPB) {      // wave-uniform
    long xrow;
    float inv_T;
    if (!locate(a, n, &xrow, &inv_T)) continue;
    const long off = ((long)a.clip * a.R + xrow) * a.C;
    const float* x = a.logits + off;
    const float* p = a.targets + n * a.ldt;
    float* d = d_logits + off;
    const float w = g * inv_T;
    if (a.mode == 0) {
      for (int y = lane; y < a.n_known; y += 64) d[y] = w * (1.f / (1.f + expf(-x[y])) - p[y]);
    } else {
      float m, s, sp = 0.f;
      softmax_stats(x, a.n_known, lane, &m, &s);
      for (int y = lane; y < a.n_known; y += 64) sp += p[y];
      sp = wave_sum(sp);
      const float k = sp / s;
      for (int y = lane; y < a.n_known; y += 64) d[y] = 0.5f * w * (expf(0.5f * x[y] - m) * k - p[y]);
    }
  }
}

// everything a launch relies on, checked on the host; N = sum of level_T on success
int check_desc(const vilco_distill_desc* d, long* N) {
  if (!d || !d->logits || !d->targets || !d->level_row || !d->level_T || !d->level_dev) return VILCO_ERR_BADARG;
  if (d->L <= 0 || d->B < 1 || d->R < 1 || d->C < 1 || d->ldt < 1) return VILCO_ERR_BADARG;
  if (d->clip < 0 || d->clip >= d->B) return VILCO_ERR_BADARG;
  if (d->n_known < 1 || d->n_known > d->C || d->n_known > d->ldt) return VILCO_ERR_BADARG;
  if (d->mode != 0 && d->mode != 1) return VILCO_ERR_BADARG;
  long n = 0;
  for (int l = 0; l < d->L; ++l) {
    const long r = d->level_row[l], T = d->level_T[l];
    if (r < 0 || T < 1 || r + T > d->R) return VILCO_ERR_BADARG;
    n += T;
  }
  *N = n;
  return VILCO_OK;
}

DistillArgs make_args(const vilco_distill_desc* d, long N) {
  DistillArgs a;
  a.logits = d->logits; a.targets = d->targets; a.level_dev = d->level_dev; a.N = N;
  a.R = d->R; a.C = d->C; a.L = d->L; a.clip = d->clip; a.ldt = d->ldt; a.n_known = d->n_known; a.mode = d->mode;
  a.coef = d->mode == 0 ? 0.01f : d->scale;
  return a;
}

}  // namespace

extern "C" size_t vilco_cl_distill_workspace(int64_t n_rows) {
  return n_rows < 0 ? 0 : (size_t)grid_blocks(n_rows) * sizeof(double) + 256;
}

extern "C" int vilco_cl_distill_fwd(const vilco_distill_desc* d, float* out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  long N = 0;
  const int rc = check_desc(d, &N);
  if (rc != VILCO_OK) return rc;
  if (!out || !workspace) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_cl_distill_workspace(N)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const DistillArgs a = make_args(d, N);
  double* part = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const int nblk = grid_blocks(N);
  hipLaunchKernelGGL(distill_fwd_kernel, dim3(nblk), dim3(DT), 0, s, a, part);
  hipLaunchKernelGGL(distill_finish_kernel, dim3(1), dim3(DT), 0, s, (const double*)part, nblk, a.coef, out);
  return vilco_launch_status();
}

extern "C" int vilco_cl_distill_bwd(const vilco_distill_desc* d, const float* g_out, float* d_logits, void* stream) {
  long N = 0;
  const int rc = check_desc(d, &N);
  if (rc != VILCO_OK) return rc;
  if (!g_out || !d_logits) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(distill_bwd_kernel, dim3(grid_blocks(N)), dim3(DT), 0, s, make_args(d, N), g_out, d_logits);
  return vilco_launch_status();
}
