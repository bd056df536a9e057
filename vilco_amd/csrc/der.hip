// Dark Experience Replay (Buzzega, Boschini, Porrello, Abati, Calderara: "Dark Experience for General Continual Learning",
// NeurIPS 2020; the reference has no logit replay, so there is no line of it to cite): the squared distance between the
// head's logits of a memory clip and the logits that clip produced when it entered the memory, and its gradient.
//
//   S = sum_{b: rec} sum_l sum_{t < V_bl} sum_{y < n_b} (x[b, row_l + t, y] - z_b[off_l + t, y])^2    (term fp32, sum fp64)
//   N = sum_{b: rec} n_b sum_l V_bl                                                                   (int64, on the device)
//   out = (float)(alpha S / N), 0 when N == 0;   c = (float)(2 alpha g / N);   d_logits = fl(fl(x - z) c) on the compared elements
//
// x = the concatenated head output [B][R][C] the label / loss kernels read (level l in rows level_row[l] .. + level_T[l],
// separator rows allowed); z_b = row b's record [sum T_l][n_b], levels end to end, n_b <= C its class count AND row stride.
// Record addresses and class counts come from der_tab in DEVICE memory ([B][2] int64: address or 0, n_b) and the valid
// lengths V_bl from level_len ([B][L] int32, what vilco_mq_loss reads), so a captured launch follows a changing table.
//
//   der_rows_kernel    one wavefront per (batch row, pyramid row) pair (a block's four waves walk pairs w, w + 4 gridDim.x, ...):
//                      rows without a record (address 0, n_b outside [1, C]) and positions at or beyond V_bl return before any
//                      load; lanes stride over the n_b classes, 16 bytes at a time where both rows are 16-byte aligned, 4 bytes
//                      otherwise; a lane adds its terms in fp64, the wave butterfly and the block's four waves add in a fixed order.
//   der_finish_kernel  one workgroup adds the partials in block order (fixed tree), forms N, writes out and N (workspace).
//   der_bwd_kernel     the same walk; every compared element of d_logits has one owner lane and is ASSIGNED; nothing else is
//                      written.  N is read from the workspace the forward filled, g from device memory.
// Two launches forward, one backward, whatever B, L and the table; no atomics: the same bits on every call.
// Bytes: 8 per compared element forward (x, z), 12 backward (x, z, d_logits).
#include "common.h"

namespace {

constexpr int DT = 256;                // threads per workgroup (4 waves)
constexpr int WPB = DT / 64;
constexpr int MAX_BLOCKS = 1024;

struct DerArgs {
  const float* logits;
  const int32_t* level_dev;            // [2][L]: first rows, lengths (the device copy of the validated host arrays)
  const int32_t* level_len;            // [B][L]
  const int64_t* der_tab;              // [B][2]
  long rows;                           // sum of level_T
  long pairs;                          // B * rows
  int B, R, C, L;
};

int grid_blocks(long pairs) {
  const long g = (pairs + WPB - 1) / WPB;
  return (int)(g < 1 ? 1 : (g > MAX_BLOCKS ? MAX_BLOCKS : g));
}

// the compared row of pair p, if any: x -> its C logits, z -> its n_b recorded logits
struct DerRow {
  long xoff;                           // element offset of the row inside [B][R][C]
  const float* z;
  int nb;
};

__device__ __forceinline__ bool locate(const DerArgs& a, long p, DerRow* r) {
  const long b = p / a.rows, n = p - b * a.rows;
  const int64_t addr = a.der_tab[2 * b], nb = a.der_tab[2 * b + 1];
  if (addr == 0 || nb < 1 || nb > a.C) return false;           // no record, or a class count that is not to be trusted
  long first = 0;
  for (int l = 0; l < a.L; ++l) {
    const int T = a.level_dev[a.L + l];
    if (T <= 0) return false;
    if (n < first + T) {
      const long t = n - first, row = (long)a.level_dev[l] + t;
      if (a.level_dev[l] < 0 || row >= a.R) return false;      // the device table disagrees with the validated bounds
      if (t >= (long)a.level_len[b * a.L + l]) return false;   // at or beyond the valid length (V <= 0: the whole level)
      r->xoff = (b * a.R + row) * a.C;
      r->z = reinterpret_cast<const float*>(addr) + n * nb;
      r->nb = (int)nb;
      return true;
    }
    first += T;
  }
  return false;
}

__device__ __forceinline__ bool aligned16(const void* p, const void* q) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}

__device__ __forceinline__ double wave_sum_f64(double v) {     // fixed butterfly, result in every lane
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double sq(float x, float z) {
  const float d = x - z;
  return (double)(d * d);
}

__global__ __launch_bounds__(DT) void der_rows_kernel(DerArgs a, double* __restrict__ part) {
  __shared__ double sw[WPB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (long p = (long)blockIdx.x * WPB + wave; p < a.pairs; p += (long)gridDim.x * WPB) {      // wave-uniform
    DerRow r;
    if (!locate(a, p, &r)) continue;
    const float* x = a.logits + r.xoff;
    const float* z = r.z;
    double v = 0.0;
    int y0 = 0;
    if (aligned16(x, z)) {
      const int nv = r.nb >> 2;
      const float4* x4 = reinterpret_cast<const float4*>(x);
      const float4* z4 = reinterpret_cast<const float4*>(z);
      for (int i = lane; i < nv; i += 64) {
        const float4 xa = x4[i], za = z4[i];
        v = v + sq(xa.x, za.x);
        v = v + sq(xa.y, za.y);
        v = v + sq(xa.z, za.z);
        v = v + sq(xa.w, za.w);
      }
      y0 = nv << 2;
    }
    for (int y = y0 + lane; y < r.nb; y += 64) v = v + sq(x[y], z[y]);
    acc = acc + wave_sum_f64(v);
  }
  if (lane == 0) sw[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = sw[0];
    for (int k = 1; k < WPB; ++k) v = v + sw[k];
    part[blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(DT) void der_finish_kernel(DerArgs a, const double* __restrict__ part, int nblk, double alpha,
                                                        float* __restrict__ out, int64_t* __restrict__ count) {
  __shared__ double sd[DT];
  __shared__ long long sn[DT];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int b = tid; b < nblk; b += DT) v = v + part[b];
  long long n = 0;
  for (int b = tid; b < a.B; b += DT) {
    const int64_t addr = a.der_tab[2 * b], nb = a.der_tab[2 * b + 1];
    if (addr == 0 || nb < 1 || nb > a.C) continue;
    long long valid = 0;
    for (int l = 0; l < a.L; ++l) {
      const int T = a.level_dev[a.L + l], V = a.level_len[b * a.L + l];
      if (T <= 0) break;                                   // the rows locate() accepts, counted the same way
      if (a.level_dev[l] < 0) continue;
      long m = (long)a.R - a.level_dev[l];
      m = m < T ? m : T;
      m = m < V ? m : V;
      valid += m < 0 ? 0 : m;
    }
    n += nb * valid;
  }
  sd[tid] = v;
  sn[tid] = n;
  __syncthreads();
  for (int o = DT / 2; o >= 1; o >>= 1) {
    if (tid < o) {
      sd[tid] = sd[tid] + sd[tid + o];
      sn[tid] = sn[tid] + sn[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    count[0] = sn[0];
    out[0] = sn[0] > 0 ? (float)(alpha * sd[0] / (double)sn[0]) : 0.f;
  }
}

__global__ __launch_bounds__(DT) void der_bwd_kernel(DerArgs a, double alpha, const float* __restrict__ g_out,
                                                     const int64_t* __restrict__ count, float* __restrict__ d_logits) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t N = count[0];
  if (N <= 0) return;
  const float c = (float)(2.0 * alpha * (double)g_out[0] / (double)N);
  for (long p = (long)blockIdx.x * WPB + wave; p < a.pairs; p += (long)gridDim.x * WPB) {      // wave-uniform
    DerRow r;
    if (!locate(a, p, &r)) continue;
    const float* x = a.logits + r.xoff;
    const float* z = r.z;
    float* d = d_logits + r.xoff;
    int y0 = 0;
    if (aligned16(x, z) && aligned16(d, d)) {
      const int nv = r.nb >> 2;
      const float4* x4 = reinterpret_cast<const float4*>(x);
      const float4* z4 = reinterpret_cast<const float4*>(z);
      float4* d4 = reinterpret_cast<float4*>(d);
      for (int i = lane; i < nv; i += 64) {
        const float4 xa = x4[i], za = z4[i];
        float4 o;
        o.x = (xa.x - za.x) * c;
        o.y = (xa.y - za.y) * c;
        o.z = (xa.z - za.z) * c;
        o.w = (xa.w - za.w) * c;
        d4[i] = o;
      }
      y0 = nv << 2;
    }
    for (int y = y0 + lane; y < r.nb; y += 64) d[y] = (x[y] - z[y]) * c;
  }
}

// everything a launch relies on, checked on the host; rows = sum of level_T on success
int check_desc(const vilco_der_desc* d, long* rows) {
  if (!d || !d->logits || !d->level_row || !d->level_T || !d->level_dev || !d->level_len || !d->der_tab) return VILCO_ERR_BADARG;
  if (d->L <= 0 || d->B <= 0 || d->R < 1 || d->C < 1) return VILCO_ERR_BADARG;
  long n = 0;
  for (int l = 0; l < d->L; ++l) {
    const long r = d->level_row[l], T = d->level_T[l];
    if (r < 0 || T < 1 || r + T > d->R) return VILCO_ERR_BADARG;
    n += T;
  }
  *rows = n;
  return VILCO_OK;
}

DerArgs make_args(const vilco_der_desc* d, long rows) {
  DerArgs a;
  a.logits = d->logits; a.level_dev = d->level_dev; a.level_len = d->level_len; a.der_tab = d->der_tab;
  a.rows = rows; a.pairs = (long)d->B * rows;
  a.B = d->B; a.R = d->R; a.C = d->C; a.L = d->L;
  return a;
}

// workspace: [N (int64) | one double per block], from the first 256-byte boundary
int64_t* ws_base(void* workspace) {
  return reinterpret_cast<int64_t*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
}

}  // namespace

extern "C" size_t vilco_der_workspace(int64_t n_pairs) {
  return n_pairs < 0 ? 0 : (size_t)(1 + grid_blocks(n_pairs)) * sizeof(double) + 256;
}

extern "C" int vilco_der_fwd(const vilco_der_desc* d, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  long rows = 0;
  const int rc = check_desc(d, &rows);
  if (rc != VILCO_OK) return rc;
  if (!out || !workspace) return VILCO_ERR_BADARG;
  const DerArgs a = make_args(d, rows);
  if (workspace_bytes < vilco_der_workspace(a.pairs)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int64_t* count = ws_base(workspace);
  double* part = reinterpret_cast<double*>(count + 1);
  const int nblk = grid_blocks(a.pairs);
  hipLaunchKernelGGL(der_rows_kernel, dim3(nblk), dim3(DT), 0, s, a, part);
  hipLaunchKernelGGL(der_finish_kernel, dim3(1), dim3(DT), 0, s, a, (const double*)part, nblk, d->alpha, out, count);
  return vilco_launch_status();
}

extern "C" int vilco_der_bwd(const vilco_der_desc* d, const float* g_out, float* d_logits, const void* workspace,
                             size_t workspace_bytes, void* stream) {
  long rows = 0;
  const int rc = check_desc(d, &rows);
  if (rc != VILCO_OK) return rc;
  if (!g_out || !d_logits || !workspace) return VILCO_ERR_BADARG;
  const DerArgs a = make_args(d, rows);
  if (workspace_bytes < vilco_der_workspace(a.pairs)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t* count = ws_base(const_cast<void*>(workspace));
  hipLaunchKernelGGL(der_bwd_kernel, dim3(grid_blocks(a.pairs)), dim3(DT), 0, s, a, d->alpha, g_out, count, d_logits);
  return vilco_launch_status();
}
