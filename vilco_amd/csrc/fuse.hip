// External classification scores fused into the MQ detections on the device: the expansion of the reference's
// postprocess_results (MQ/libs/utils/postprocessing.py:97-155), feeding vilco_det_ap without a host round trip.
// Per video: keep the num_pred best rows by score, take the topk best classes of the video's class-score vector, emit
// topk x rows new rows -- class by rank, inside a class the kept rows by rank -- with label = the class,
// score = sqrt(class score * row score) and the row's segment.
//
// One workgroup per video.  Both rankings are counting ranks over order-preserving integer keys: rank(i) = number of j
// with key_j > key_i, or key_j == key_i and j > i -- descending value, equal values (and NaN, which ranks first as in
// np.argsort(x)[::-1]) with the later index first, the reverse of a stable ascending sort.  The row keys and the slot
// table live in LDS (videos of more than LDS_ROWS rows use their slice of the workspace instead).  The fused score is one
// fp64 product and one correctly rounded fp64 square root, so it is bit-equal to NumPy's; a negative product gives NaN.
// No atomics: repeated calls are bitwise equal.
#include "common.h"

namespace {

constexpr int FT = 256;              // threads per workgroup
constexpr int LDS_ROWS = 4096;       // rows of a video ranked out of LDS
constexpr int MAX_TOPK = 64;

// total order of a double as an unsigned integer: NaN above +inf (numpy sorts NaN last), -0 == +0
__device__ __forceinline__ unsigned long long ord_bits(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) x = 0.0;
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

__global__ __launch_bounds__(FT) void fuse_kernel(const double* __restrict__ score, const double* __restrict__ ts,
                                                  const double* __restrict__ te, const int* __restrict__ pred_off,
                                                  const double* __restrict__ cls_score, int n_cls, int num_pred, int topk,
                                                  const int* __restrict__ out_off, unsigned long long* __restrict__ gkeys,
                                                  int* __restrict__ gsel, int* __restrict__ out_vid,
                                                  int* __restrict__ out_label, double* __restrict__ out_ts,
                                                  double* __restrict__ out_te, double* __restrict__ out_score) {
  __shared__ unsigned long long lkeys[LDS_ROWS];
  __shared__ int lsel[LDS_ROWS];
  __shared__ int csel[MAX_TOPK];
  __shared__ double cval[MAX_TOPK];
  const int v = blockIdx.x, tid = threadIdx.x;
  const int p0 = pred_off[v], n = pred_off[v + 1] - p0;
  const int m = n < num_pred ? n : num_pred;
  const long o0 = out_off[v];
  unsigned long long* keys = n <= LDS_ROWS ? lkeys : gkeys + p0;
  int* sel = n <= LDS_ROWS ? lsel : gsel + p0;
  for (int i = tid; i < n; i += FT) keys[i] = ord_bits(score[p0 + i]);
  // the topk best classes; the vector is short, every lane reads the same element at a time
  const double* cs = cls_score + (long)v * n_cls;
  for (int i = tid; i < n_cls; i += FT) {
    const double x = cs[i];
    const unsigned long long k = ord_bits(x);
    int r = 0;
    for (int j = 0; j < n_cls; ++j) {
      const unsigned long long kj = ord_bits(cs[j]);
      r += (kj > k || (kj == k && j > i)) ? 1 : 0;
    }
    if (r < topk) { csel[r] = i; cval[r] = x; }
  }
  __syncthreads();
  // slot r of the kept rows = the row of rank r
  for (int i = tid; i < n; i += FT) {
    const unsigned long long k = keys[i];
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const unsigned long long kj = keys[j];
      r += (kj > k || (kj == k && j > i)) ? 1 : 0;
    }
    if (r < m) sel[r] = i;
  }
  __syncthreads();
  // consecutive lanes write consecutive output rows
  const int total = topk * m;
  for (int idx = tid; idx < total; idx += FT) {
    const int c = idx / m, r = idx - c * m;
    const int row = p0 + sel[r];
    const long o = o0 + idx;
    out_vid[o] = v;
    out_label[o] = csel[c];
    out_ts[o] = ts[row];
    out_te[o] = te[row];
    out_score[o] = __dsqrt_rn(cval[c] * score[row]);
  }
}

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace

extern "C" size_t vilco_score_fuse_workspace(int64_t n_pred, int32_t n_vid) {
  if (n_pred < 0 || n_vid < 0 || n_pred > 0x7ffffffeL) return 0;
  const size_t rows = (size_t)(n_pred > 0 ? n_pred : 1);
  return 2 * al256(((size_t)n_vid + 1) * 4) + al256(rows * 8) + al256(rows * 4) + 256;
}

extern "C" int vilco_score_fuse(const double* pred_score, const double* pred_start, const double* pred_end,
                                const int32_t* pred_off, int64_t n_pred, int32_t n_vid, const double* cls_score,
                                int32_t n_cls, int32_t num_pred, int32_t topk, const int32_t* out_off, int64_t n_out,
                                int32_t* out_vid, int32_t* out_label, double* out_start, double* out_end, double* out_score,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (n_pred < 0 || n_vid < 0 || n_cls < 0 || n_out < 0) return VILCO_ERR_BADARG;
  if (topk < 1 || num_pred < 1 || topk > n_cls) return VILCO_ERR_BADARG;
  if (!pred_off || !out_off || !workspace) return VILCO_ERR_BADARG;
  if (n_vid > 0 && !cls_score) return VILCO_ERR_BADARG;
  if (n_pred > 0 && (!pred_score || !pred_start || !pred_end)) return VILCO_ERR_BADARG;
  if (n_out > 0 && (!out_vid || !out_label || !out_start || !out_end || !out_score)) return VILCO_ERR_BADARG;
  if (topk > MAX_TOPK || n_pred > 0x7ffffffeL || n_out > 0x7ffffffeL) return VILCO_ERR_UNSUPPORTED;
  // the offset tables are host arrays: every row the kernel touches is checked here
  if (pred_off[0] != 0 || out_off[0] != 0) return VILCO_ERR_BADARG;
  for (int v = 0; v < n_vid; ++v) {
    const int64_t n = (int64_t)pred_off[v + 1] - pred_off[v];
    if (n < 0) return VILCO_ERR_BADARG;
    const int64_t m = n < num_pred ? n : num_pred;
    if ((int64_t)out_off[v + 1] - out_off[v] != (int64_t)topk * m) return VILCO_ERR_BADARG;
  }
  if (pred_off[n_vid] != n_pred || out_off[n_vid] != n_out) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_score_fuse_workspace(n_pred, n_vid)) return VILCO_ERR_WORKSPACE;
  if (n_vid == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const size_t tab = ((size_t)n_vid + 1) * 4, rows = (size_t)(n_pred > 0 ? n_pred : 1);
  int* d_pred_off = reinterpret_cast<int*>(base);
  int* d_out_off = reinterpret_cast<int*>(base + al256(tab));
  unsigned long long* gkeys = reinterpret_cast<unsigned long long*>(base + 2 * al256(tab));
  int* gsel = reinterpret_cast<int*>(base + 2 * al256(tab) + al256(rows * 8));
  if (hipMemcpyAsync(d_pred_off, pred_off, tab, hipMemcpyHostToDevice, s) != hipSuccess) return VILCO_ERR_LAUNCH;
  if (hipMemcpyAsync(d_out_off, out_off, tab, hipMemcpyHostToDevice, s) != hipSuccess) return VILCO_ERR_LAUNCH;
  hipLaunchKernelGGL(fuse_kernel, dim3(n_vid), dim3(FT), 0, s, pred_score, pred_start, pred_end, d_pred_off, cls_score,
                     (int)n_cls, (int)num_pred, (int)topk, d_out_off, gkeys, gsel, out_vid, out_label, out_start, out_end,
                     out_score);
  return vilco_launch_status();
}
