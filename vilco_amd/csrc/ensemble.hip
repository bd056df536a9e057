// NLQ model ensembling on the device: the per-query recipe of the reference's challenge submission (NLQ/ensemble.py:7-101,
// 123-143 with NLQ/temporal_nms.py:6-74) for all queries in one launch.  Per query: the first top1_max_input rows of every
// model are clustered by their centres into new proposals (top1_generator), the proposals are appended to the first
// max_input rows of every model, and a greedy temporal NMS over that list keeps max_after_nms rows, padded with the last.
//
// One wavefront per query, EQ queries per workgroup, the query's rows in the wave's own slice of LDS.  Every ordering is a
// counting rank (the number of rows that come first), which is what a stable sort produces: centres ascending (unique after
// the dict step), proposals by cluster total descending with the earlier cluster first, candidates by score descending
// with the earlier position first.  Clusters are read off a ballot of "the gap to the previous centre is not below
// `distance`"; the lane of a cluster's first centre walks the cluster left to right.  The NMS is at most max_after_nms
// rounds of "lowest rank still alive" (ballot + ffs), the head read from LDS by every lane, every lane testing its own two
// candidates.  All arithmetic is fp64 in the reference's operation order (compiled with -ffp-contract=off), so the result
// is bit-equal to CPython's.  No atomics, no workspace, no host synchronisation: repeated calls are bitwise equal.
#include "common.h"

namespace {

constexpr int EQ = 4;                 // queries (wavefronts) per workgroup
constexpr int ET = EQ * VILCO_WAVE;   // threads per workgroup
constexpr int ENS_MODELS = 8;
constexpr int ENS_INPUT = 10;
constexpr int ENS_TOP1 = 64;          // rows the generator sees: one per lane
constexpr int ENS_CAND = 128;         // rows the NMS sees: two per lane

struct EnsWave {                      // one wavefront's LDS
  double cs[ENS_CAND], ce[ENS_CAND], cw[ENS_CAND];   // the fusion list: start, end, score
  double ss[ENS_CAND], se[ENS_CAND], sw[ENS_CAND];   // the same, ordered by score
  double tc[ENS_TOP1];                               // generator: centres in input order
  double gc[ENS_TOP1], gs[ENS_TOP1], ge[ENS_TOP1], gw[ENS_TOP1];   // generator: rows in centre order
  double ps[ENS_TOP1], pe[ENS_TOP1], pw[ENS_TOP1], pt[ENS_TOP1];   // proposals in cluster order; pt = cluster total
};

// the reference's "iou": intersection over the span, 0 for an empty span
__device__ __forceinline__ double span_overlap(double s1, double e1, double s2, double e2) {
  const double lo = (e1 < e2 ? e1 : e2) - (s1 > s2 ? s1 : s2);
  const double inter = lo > 0.0 ? lo : 0.0;
  const double span = (e1 > e2 ? e1 : e2) - (s1 < s2 ? s1 : s2);
  return span == 0.0 ? 0.0 : inter / span;
}

template <typename T>
__global__ __launch_bounds__(ET) void ensemble_kernel(const T* __restrict__ pred, const int* __restrict__ cnt, int n_model,
                                                      long n_query, int k_cap, int max_input, int top1, double distance,
                                                      double nms_thd, int max_after, int pad, double* __restrict__ out,
                                                      int* __restrict__ out_cnt, double* __restrict__ prop,
                                                      int* __restrict__ prop_cnt) {
  __shared__ EnsWave lds[EQ];
  const int lane = threadIdx.x % VILCO_WAVE;
  EnsWave& w = lds[threadIdx.x / VILCO_WAVE];
  const long q = (long)blockIdx.x * EQ + threadIdx.x / VILCO_WAVE;
  const bool live = q < n_query;          // the waves of a tail workgroup take part in the barriers with nothing to do

  // rows every model brings: c = cnt clamped to [0, k_cap]; the fusion list starts with min(c, max_input) rows per model
  int base = 0;                           // rows of the fusion list before the proposals
  int my_off[2] = {0, 0};                 // position of this lane's model rows in the fusion list
  bool my_ok[2] = {false, false};
  int my_m[2], my_r[2];
  for (int k = 0; k < 2; ++k) {
    const int i = lane + k * VILCO_WAVE;
    my_m[k] = i / max_input;
    my_r[k] = i - my_m[k] * max_input;
  }
  int t_cnt = 0;                          // rows this lane's model gives the generator
  const int t_m = top1 > 0 ? lane / top1 : 0, t_r = top1 > 0 ? lane - t_m * top1 : 0;
  if (live) {
    for (int m = 0; m < n_model; ++m) {
      int c = cnt[(long)m * n_query + q];
      c = c < 0 ? 0 : (c > k_cap ? k_cap : c);
      const int take = c < max_input ? c : max_input;
      for (int k = 0; k < 2; ++k)
        if (my_m[k] == m) { my_off[k] = base + my_r[k]; my_ok[k] = my_r[k] < take; }
      if (t_m == m) t_cnt = c < top1 ? c : top1;
      base += take;
    }
  }

  // ---- the generator: one row per lane, in the order of the concatenation
  const bool t_ok = live && top1 > 0 && t_m < n_model && t_r < t_cnt;
  double ts = 0.0, te = 0.0, tw = 0.0, tcen = 0.0;
  if (t_ok) {
    const T* p = pred + (((long)t_m * n_query + q) * k_cap + t_r) * 3;
    ts = (double)p[0]; te = (double)p[1]; tw = (double)p[2];
    tcen = (te + ts) / 2.0;
    w.tc[lane] = tcen;
  }
  const unsigned long long t_mask = __ballot(t_ok);
  __syncthreads();
  // the dict keyed by centre: of equal centres the last row stays
  bool t_keep = t_ok;
  if (t_ok) {
    unsigned long long later = t_mask & ~((2ull << lane) - 1ull);
    while (later) {
      const int j = __ffsll((long long)later) - 1;
      later &= later - 1;
      if (w.tc[j] == tcen) { t_keep = false; break; }
    }
  }
  const unsigned long long k_mask = __ballot(t_keep);
  const int n_cen = __popcll(k_mask);
  if (t_keep) {                           // centres ascending: they are distinct, the rank is the position
    int r = 0;
    unsigned long long rest = k_mask;
    while (rest) {
      const int j = __ffsll((long long)rest) - 1;
      rest &= rest - 1;
      r += w.tc[j] < tcen ? 1 : 0;
    }
    w.gc[r] = tcen; w.gs[r] = ts; w.ge[r] = te; w.gw[r] = tw;
  }
  __syncthreads();
  // chains: a centre opens a cluster unless its gap to the previous centre is below `distance`
  const bool in_c = lane < n_cen;
  const bool opens = in_c && (lane == 0 || !(w.gc[lane] - w.gc[lane - 1] < distance));
  const unsigned long long o_mask = __ballot(opens);
  const int n_prop = __popcll(o_mask);
  if (opens) {
    const unsigned long long after = o_mask & ~((2ull << lane) - 1ull);
    const int end = after ? __ffsll((long long)after) - 1 : n_cen;
    const int c = end - lane;
    double total = 0.0, best = w.gw[lane];
    int arg = lane;
    for (int j = lane; j < end; ++j) {    // the sum left to right from 0, the first maximum
      const double x = w.gw[j];
      total = total + x;
      if (x > best) { best = x; arg = j; }
    }
    int mid = lane + (c - 1) / 2;         // odd: the middle; even: the upper middle only if its score is greater
    if ((c & 1) == 0) mid = w.gw[lane + c / 2] > w.gw[lane + c / 2 - 1] ? lane + c / 2 : lane + c / 2 - 1;
    const int g = __popcll(o_mask & ((1ull << lane) - 1ull));
    w.ps[g] = (w.gs[mid] + w.gs[arg]) / 2.0;
    w.pe[g] = (w.ge[mid] + w.ge[arg]) / 2.0;
    w.pw[g] = (w.gw[mid] + w.gw[arg]) / 2.0;
    w.pt[g] = total;
  }
  // the model rows of the fusion list
  for (int k = 0; k < 2; ++k)
    if (my_ok[k]) {
      const T* p = pred + (((long)my_m[k] * n_query + q) * k_cap + my_r[k]) * 3;
      w.cs[my_off[k]] = (double)p[0]; w.ce[my_off[k]] = (double)p[1]; w.cw[my_off[k]] = (double)p[2];
    }
  __syncthreads();
  // proposals by total, descending, equal totals in cluster order; they follow the model rows
  if (lane < n_prop) {
    const double t = w.pt[lane];
    int r = 0;
    for (int j = 0; j < n_prop; ++j) {
      const double x = w.pt[j];
      r += (x > t || (x == t && j < lane)) ? 1 : 0;
    }
    w.cs[base + r] = w.ps[lane]; w.ce[base + r] = w.pe[lane]; w.cw[base + r] = w.pw[lane];
    if (prop) {
      double* o = prop + ((long)q * n_model * top1 + r) * 4;
      o[0] = w.ps[lane]; o[1] = w.pe[lane]; o[2] = w.pw[lane]; o[3] = t;
    }
  }
  if (live && prop_cnt && lane == 0) prop_cnt[q] = n_prop;
  const int n = base + n_prop;            // <= ENS_CAND: checked on the host
  __syncthreads();
  // by score, descending, equal scores in list order
  for (int k = 0; k < 2; ++k) {
    const int i = lane + k * VILCO_WAVE;
    if (i < n) {
      const double x = w.cw[i];
      int r = 0;
      for (int j = 0; j < n; ++j) {
        const double y = w.cw[j];
        r += (y > x || (y == x && j < i)) ? 1 : 0;
      }
      w.ss[r] = w.cs[i]; w.se[r] = w.ce[i]; w.sw[r] = x;
    }
  }
  __syncthreads();
  if (!live) return;
  // greedy NMS: this lane owns ranks lane and lane + 64
  const bool in0 = lane < n, in1 = lane + VILCO_WAVE < n;
  const double s0 = in0 ? w.ss[lane] : 0.0, e0 = in0 ? w.se[lane] : 0.0;
  const double s1 = in1 ? w.ss[lane + VILCO_WAVE] : 0.0, e1 = in1 ? w.se[lane + VILCO_WAVE] : 0.0;
  bool a0 = in0, a1 = in1;
  double* o = out + (long)q * max_after * 3;
  double hs = 0.0, he = 0.0, hw = 0.0;
  int kept = 0;
  while (kept < max_after) {
    const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
    if (!(m0 | m1)) break;
    const int head = m0 ? __ffsll((long long)m0) - 1 : VILCO_WAVE + __ffsll((long long)m1) - 1;
    hs = w.ss[head]; he = w.se[head]; hw = w.sw[head];
    if (lane == 0) { o[kept * 3] = hs; o[kept * 3 + 1] = he; o[kept * 3 + 2] = hw; }
    if (head == lane) a0 = false;
    if (head == lane + VILCO_WAVE) a1 = false;
    if (a0 && span_overlap(hs, he, s0, e0) > nms_thd) a0 = false;
    if (a1 && span_overlap(hs, he, s1, e1) > nms_thd) a1 = false;
    ++kept;
  }
  if (lane == 0) out_cnt[q] = kept;
  // the rest of the table: the last kept row again, or zeros without padding (and for a query without rows)
  if (!pad || kept == 0) hs = he = hw = 0.0;
  for (int r = kept + lane; r < max_after; r += VILCO_WAVE) { o[r * 3] = hs; o[r * 3 + 1] = he; o[r * 3 + 2] = hw; }
}

}  // namespace

extern "C" int vilco_nlq_ensemble(const void* pred, int32_t pred_fp32, const int32_t* cnt, int32_t n_model, int64_t n_query,
                                  int32_t k_cap, int32_t max_input, int32_t top1_max_input, double distance, double nms_thd,
                                  int32_t max_after_nms, int32_t pad, double* out, int32_t* out_cnt, double* prop,
                                  int32_t* prop_cnt, void* stream) {
  if (n_model < 1 || n_model > ENS_MODELS || n_query < 0 || n_query > 0x7ffffffeL) return VILCO_ERR_BADARG;
  if (max_input < 1 || max_input > ENS_INPUT || k_cap < max_input) return VILCO_ERR_BADARG;
  if (top1_max_input < 0 || (int64_t)n_model * top1_max_input > ENS_TOP1) return VILCO_ERR_BADARG;
  const int top1_rows = top1_max_input < k_cap ? top1_max_input : k_cap;          // a model has at most k_cap rows
  if (n_model * max_input + n_model * top1_rows > ENS_CAND) return VILCO_ERR_BADARG;
  if (max_after_nms < 1 || max_after_nms > ENS_CAND) return VILCO_ERR_BADARG;
  if ((prop == nullptr) != (prop_cnt == nullptr)) return VILCO_ERR_BADARG;
  if (n_query > 0 && (!pred || !cnt || !out || !out_cnt)) return VILCO_ERR_BADARG;
  if (!vilco_aligned(pred, pred_fp32 ? 4 : 8) || !vilco_aligned(out, 8) || !vilco_aligned(prop, 8)) return VILCO_ERR_BADARG;
  if (n_query == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((n_query + EQ - 1) / EQ));
  if (pred_fp32)
    hipLaunchKernelGGL(ensemble_kernel<float>, grid, dim3(ET), 0, s, reinterpret_cast<const float*>(pred), cnt, (int)n_model,
                       (long)n_query, (int)k_cap, (int)max_input, (int)top1_max_input, distance, nms_thd, (int)max_after_nms,
                       (int)(pad != 0), out, out_cnt, prop, prop_cnt);
  else
    hipLaunchKernelGGL(ensemble_kernel<double>, grid, dim3(ET), 0, s, reinterpret_cast<const double*>(pred), cnt,
                       (int)n_model, (long)n_query, (int)k_cap, (int)max_input, (int)top1_max_input, distance, nms_thd,
                       (int)max_after_nms, (int)(pad != 0), out, out_cnt, prop, prop_cnt);
  return vilco_launch_status();
}
