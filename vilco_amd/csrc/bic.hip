// BiC stage 2 (bias correction, Wu et al. 2019): fit alpha, beta of the newest BiasLayer on held-out clips with the network
// frozen -- the reference's second phase, MQ/train_bic.py:602-649 (whose bias optimizer, :622, is never stepped) with
// train_bic_one_epoch's forward + losses + backward per step.  A frozen network's raw logits never change, so the Python
// side caches them once (vilco_amd/cl_methods/bic.py) and a step is one read of the newest split's columns:
//
//   L = (1 / max(P, 1)) sum_{n in S} weight[n] sum_{c in [lo, hi)} focal(alpha x[n, c] + beta, t[n, c]),  P = sum_{n in S} pos[n]
//
//   bic_part_kernel    grid (gx, gy): the blocks of column y walk the step's clips y, y + gy, ...; inside a clip the
//                      (row, column) elements of the [rows, hi - lo) window are dealt to the threads in flat order, so a
//                      wave reads runs of hi - lo consecutive floats with 4-byte loads -- any lo, nothing outside a row, no
//                      alignment to respect.  fp32 per element; every thread adds its elements in fp64, a butterfly adds
//                      the wave, the four waves are added in order: one (L, dL/dalpha, dL/dbeta, P) partial per block.
//   bic_finish_kernel  one workgroup adds the partials in block order (fixed tree), divides by max(P, 1) and either
//                      writes the three values (vilco_bic_eval) or takes the SGD step on the fp64 master copy of
//                      (alpha, beta), writes loss_out[k] and the fp32 (alpha, beta) the next step's elements use.
// vilco_bic_fit enqueues the pair once per step: the steps depend on each other through stream order alone -- no grid
// barrier, no spinning, no atomics, no host synchronisation; repeated calls are bit-equal.
#include "common.h"

namespace {

constexpr int BT = 256;                // threads per workgroup (4 waves)
constexpr int EPT = 8;                 // elements per thread the grid is sized for
constexpr int MAX_GY = 64;
constexpr int MAX_BLOCKS = 1024;
constexpr long MAX_ROWS = (1l << 31) / 128 - 1;      // rows * (hi - lo) stays below 2^31

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

struct Plan { int gx, gy; };

Plan plan(long N, int n_clips, int nslot, int W) {
  Plan p;
  p.gy = nslot < MAX_GY ? (nslot < 1 ? 1 : nslot) : MAX_GY;
  const long per_clip = (N + (n_clips > 0 ? n_clips : 1) - 1) / (n_clips > 0 ? n_clips : 1);
  long gx = (per_clip * W + (long)BT * EPT - 1) / ((long)BT * EPT);
  const long cap = MAX_BLOCKS / p.gy;
  p.gx = (int)(gx < 1 ? 1 : (gx > cap ? cap : gx));
  return p;
}

size_t ws_bytes(Plan p) { return 256 + al256((size_t)p.gx * p.gy * 4 * sizeof(double)) + 256; }

// sigmoid_focal_loss (alpha 0.25, gamma 2) of logit z against target t and its derivative in z
__device__ __forceinline__ float focal_dz(float z, float t, float* dz) {
  const float p = 1.f / (1.f + expf(-z));
  const float ce = fmaxf(z, 0.f) - z * t + log1pf(expf(-fabsf(z)));
  const float q = p + t - 2.f * p * t;                      // 1 - p_t
  const float al = 0.25f * t + 0.75f * (1.f - t);
  *dz = al * ((p - t) * q * q + ce * 2.f * q * (1.f - 2.f * t) * p * (1.f - p));
  return al * ce * q * q;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// order: the step's clip list (null: clips 0 .. nslot-1).  ab64: the fit's master copy (null: ab32 is read)
__global__ __launch_bounds__(BT) void bic_part_kernel(const float* __restrict__ logits, const unsigned long long* __restrict__ bits,
                                                      const float* __restrict__ weight, const unsigned char* __restrict__ pos,
                                                      const int* __restrict__ clip_ptr, const int* __restrict__ order, int nslot,
                                                      int n_clips, long N, int C, int lo, int W, float smoothing,
                                                      const double* __restrict__ ab64, const float* __restrict__ ab32,
                                                      double* __restrict__ part) {
  __shared__ double sw[4][BT / 64];
  const int tid = threadIdx.x;
  const float alpha = ab64 ? (float)ab64[0] : ab32[0];
  const float beta = ab64 ? (float)ab64[1] : ab32[1];
  const float t_on = (1.f - smoothing) + smoothing / (float)(C + 1), t_off = smoothing / (float)(C + 1);
  double sl = 0.0, sa = 0.0, sb = 0.0, sp = 0.0;
  for (int s = blockIdx.y; s < nslot; s += gridDim.y) {
    const int clip = order ? order[s] : s;
    if (clip < 0 || clip >= n_clips) continue;               // a bad index reads nothing
    long r0 = clip_ptr[clip], r1 = clip_ptr[clip + 1];
    if (r0 < 0) r0 = 0;
    if (r1 > N) r1 = N;
    if (r1 <= r0) continue;                                  // empty clip
    const int ne = (int)(r1 - r0) * W;
    for (int e = blockIdx.x * BT + tid; e < ne; e += gridDim.x * BT) {
      const int r = e / W, j = e - r * W;
      const long row = r0 + r;
      const int c = lo + j;
      const float x = logits[row * C + c];
      const float w = weight[row];
      const float t = ((bits[row * 2 + (c >> 6)] >> (c & 63)) & 1ull) ? t_on : t_off;
      float dz;
      const float f = focal_dz(alpha * x + beta, t, &dz);
      const float g = w * dz;
      sl = sl + (double)(w * f);
      sa = sa + (double)(g * x);
      sb = sb + (double)g;
      if (j == 0) sp = sp + (double)pos[row];
    }
  }
  sl = wave_sum_f64(sl); sa = wave_sum_f64(sa); sb = wave_sum_f64(sb); sp = wave_sum_f64(sp);
  if ((tid & 63) == 0) { sw[0][tid >> 6] = sl; sw[1][tid >> 6] = sa; sw[2][tid >> 6] = sb; sw[3][tid >> 6] = sp; }
  __syncthreads();
  if (tid < 4) {
    double v = sw[tid][0];
    for (int k = 1; k < BT / 64; ++k) v = v + sw[tid][k];
    part[(long)(blockIdx.y * gridDim.x + blockIdx.x) * 4 + tid] = v;
  }
}

// out != null: out[0..2] = L, dL/dalpha, dL/dbeta.  Otherwise one SGD step on ab64, loss_out[step] and the fp32 copy.
__global__ __launch_bounds__(BT) void bic_finish_kernel(const double* __restrict__ part, int nblk, double lr, double* __restrict__ ab64,
                                                        float* __restrict__ ab32, double* __restrict__ loss_out, int step,
                                                        double* __restrict__ out) {
  __shared__ double sd[4][BT];
  const int tid = threadIdx.x;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = tid; b < nblk; b += BT)
    for (int q = 0; q < 4; ++q) v[q] = v[q] + part[(long)b * 4 + q];
  for (int q = 0; q < 4; ++q) sd[q][tid] = v[q];
  __syncthreads();
  for (int o = BT / 2; o >= 1; o >>= 1) {
    if (tid < o)
      for (int q = 0; q < 4; ++q) sd[q][tid] = sd[q][tid] + sd[q][tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double P = sd[3][0] > 1.0 ? sd[3][0] : 1.0;
    const double L = sd[0][0] / P, ga = sd[1][0] / P, gb = sd[2][0] / P;
    if (out) {
      out[0] = L; out[1] = ga; out[2] = gb;
    } else {
      const double a = ab64[0] - lr * ga, b = ab64[1] - lr * gb;
      ab64[0] = a; ab64[1] = b;
      ab32[0] = (float)a; ab32[1] = (float)b;
      loss_out[step] = L;
    }
  }
}

__global__ void bic_init_kernel(const float* __restrict__ ab32, double* __restrict__ ab64) {
  if (threadIdx.x < 2) ab64[threadIdx.x] = (double)ab32[threadIdx.x];
}

int check_common(const void* logits, const void* bits, const void* weight, const void* pos, const void* clip_ptr, int64_t N,
                 int32_t n_clips, int32_t C, int32_t lo, int32_t hi) {
  if (N < 0 || n_clips < 0 || C < 1 || C > 128 || lo < 0 || lo >= hi || hi > C) return VILCO_ERR_BADARG;
  if (!clip_ptr || (N > 0 && (!logits || !bits || !weight || !pos))) return VILCO_ERR_BADARG;
  if (N > MAX_ROWS) return VILCO_ERR_UNSUPPORTED;
  return VILCO_OK;
}

double* ws_base(void* ws) { return reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(ws) + 255) / 256 * 256); }

}  // namespace

extern "C" size_t vilco_bic_fit_ws_bytes(int64_t N, int32_t n_clips, int32_t batch_clips, int32_t lo, int32_t hi) {
  if (N < 0 || n_clips < 0 || batch_clips <= 0 || lo < 0 || lo >= hi || hi > 128) return 0;
  return ws_bytes(plan(N, n_clips, batch_clips, hi - lo));
}

extern "C" size_t vilco_bic_eval_ws_bytes(int64_t N, int32_t n_clips, int32_t lo, int32_t hi) {
  if (N < 0 || n_clips < 0 || lo < 0 || lo >= hi || hi > 128) return 0;
  return ws_bytes(plan(N, n_clips, n_clips, hi - lo));
}

extern "C" int vilco_bic_fit(const float* logits, const uint64_t* label_bits, const float* weight, const uint8_t* pos,
                             const int32_t* clip_ptr, int64_t N, int32_t n_clips, const int32_t* order, int32_t n_steps,
                             int32_t batch_clips, int32_t C, int32_t lo, int32_t hi, float smoothing, double lr,
                             float* ab_inout, double* loss_out, void* ws, size_t ws_size, void* stream) {
  const int rc = check_common(logits, label_bits, weight, pos, clip_ptr, N, n_clips, C, lo, hi);
  if (rc != VILCO_OK) return rc;
  if (batch_clips <= 0 || n_steps < 0 || !ab_inout) return VILCO_ERR_BADARG;
  if (n_steps > 0 && (!order || !loss_out || !ws)) return VILCO_ERR_BADARG;
  if (ws_size < vilco_bic_fit_ws_bytes(N, n_clips, batch_clips, lo, hi)) return VILCO_ERR_WORKSPACE;
  if (n_steps == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Plan p = plan(N, n_clips, batch_clips, hi - lo);
  double* ab64 = ws_base(ws);
  double* part = ab64 + 32;
  hipLaunchKernelGGL(bic_init_kernel, dim3(1), dim3(64), 0, s, ab_inout, ab64);
  for (int k = 0; k < n_steps; ++k) {
    hipLaunchKernelGGL(bic_part_kernel, dim3(p.gx, p.gy), dim3(BT), 0, s, logits,
                       reinterpret_cast<const unsigned long long*>(label_bits), weight, pos, clip_ptr,
                       order + (long)k * batch_clips, (int)batch_clips, (int)n_clips, (long)N, (int)C, (int)lo, (int)(hi - lo),
                       smoothing, (const double*)ab64, (const float*)nullptr, part);
    hipLaunchKernelGGL(bic_finish_kernel, dim3(1), dim3(BT), 0, s, (const double*)part, p.gx * p.gy, lr, ab64, ab_inout,
                       loss_out, k, (double*)nullptr);
  }
  return vilco_launch_status();
}

extern "C" int vilco_bic_eval(const float* logits, const uint64_t* label_bits, const float* weight, const uint8_t* pos,
                              const int32_t* clip_ptr, int64_t N, int32_t n_clips, int32_t C, int32_t lo, int32_t hi,
                              float smoothing, const float* ab, double* out3, void* ws, size_t ws_size, void* stream) {
  const int rc = check_common(logits, label_bits, weight, pos, clip_ptr, N, n_clips, C, lo, hi);
  if (rc != VILCO_OK) return rc;
  if (!ab || !out3 || !ws) return VILCO_ERR_BADARG;
  if (ws_size < vilco_bic_eval_ws_bytes(N, n_clips, lo, hi)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const Plan p = plan(N, n_clips, n_clips, hi - lo);
  double* part = ws_base(ws) + 32;
  hipLaunchKernelGGL(bic_part_kernel, dim3(p.gx, p.gy), dim3(BT), 0, s, logits,
                     reinterpret_cast<const unsigned long long*>(label_bits), weight, pos, clip_ptr, (const int*)nullptr,
                     (int)n_clips, (int)n_clips, (long)N, (int)C, (int)lo, (int)(hi - lo), smoothing, (const double*)nullptr, ab,
                     part);
  hipLaunchKernelGGL(bic_finish_kernel, dim3(1), dim3(BT), 0, s, (const double*)part, p.gx * p.gy, 0.0, (double*)nullptr,
                     (float*)nullptr, (double*)nullptr, 0, out3);
  return vilco_launch_status();
}
