// MQ and NLQ evaluation on the device: detection AP over tIoU thresholds (MQ/libs/utils/metrics.py:274-393) and Recall@K over tIoU
// (MQ/libs/utils/get_retrieval_performance.py:116-184).  Every tIoU, precision and recall value is fp64 in the reference's
// expression order and this file is compiled with -ffp-contract=off, so match decisions are bit-identical.
//
// Detection AP, per call:
//   rank     LSD radix sort (8-bit digits, one item per thread, stable) of the prediction indices: start from the reversed
//            input order, sort by the descending score key, then by class.  Result: perm1 = per class, score descending,
//            ties (and NaN, which comes first) with the later row first -- the reverse of a stable ascending sort.
//   group    the same sort continued from perm1 by video, then by class: perm2 = (class, video) groups in rank order.
//   match    one wavefront per (class, video) ground-truth group.  Its predictions are visited in rank order; per
//            threshold the first unlocked GT in the reference's order (NaN tIoU first, then tIoU descending, later GT
//            first on ties) among those that do not fail `tiou < thr` is locked and the prediction is a TP.
//   ap       one workgroup per (class, threshold): integer prefix counts of the TP flags in rank order, fp64 precision /
//            recall, the reverse running maximum and the sum of interpolated_prec_rec, in fixed order.  A class without
//            ground truth (cls_npos == 0) has no group, hence no TP and no term: AP 0.  The reference cannot reach that
//            state (its class index is built from the GT labels), so 0 is this library's documented value.
// No float atomics, no allocation, no host synchronisation; workgroups meet only at launch boundaries.
// NLQ Recall@K over IoU and mIoU (NLQ/libs/utils/metrics.py:47-68, 107-177): see the section further down.
#include "common.h"

namespace {

constexpr int RT = 256;              // radix sort: threads (= items) per tile
constexpr int VID_BITS = 24;         // (class, video) key: class << 24 | video
constexpr int MAX_THR = 16;
constexpr int MAX_RANK = 8;

struct Thr { double t[MAX_THR]; };
struct Ranks { int r[MAX_RANK]; };

enum { KEY_SCORE = 0, KEY_CLS = 1, KEY_VID = 2 };

struct PredKeys {
  const int* vid; const int* cls; const double* score;
  int n_cls, n_vid;
};

// total order of a double as an unsigned integer: NaN above +inf (numpy sorts NaN last), -0 == +0
__device__ __forceinline__ unsigned long long ord_bits(double x) {
  if (x != x) return ~0ull;
  if (x == 0.0) x = 0.0;
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

__device__ __forceinline__ int cls_key(const PredKeys& k, int row) {
  const int c = k.cls[row];
  return (c >= 0 && c < k.n_cls) ? c : k.n_cls;          // out-of-range labels sort last and are ignored
}
__device__ __forceinline__ int vid_key(const PredKeys& k, int row) {
  const int v = k.vid[row];
  return (v >= 0 && v < k.n_vid) ? v : k.n_vid;          // videos without ground truth: every prediction is an FP
}

__device__ __forceinline__ unsigned digit_of(const PredKeys& k, int mode, int shift, int row) {
  if (mode == KEY_SCORE) return (unsigned)((~ord_bits(k.score[row]) >> shift) & 255ull);
  const int v = mode == KEY_CLS ? cls_key(k, row) : vid_key(k, row);
  return ((unsigned)v >> shift) & 255u;
}

__global__ __launch_bounds__(RT) void ev_iota_rev_kernel(int* __restrict__ idx, int n) {
  const int i = blockIdx.x * RT + threadIdx.x;
  if (i < n) idx[i] = n - 1 - i;
}

// hist[d * nblk + b] = items of tile b with digit d
__global__ __launch_bounds__(RT) void ev_hist_kernel(const int* __restrict__ src, int n, PredKeys k, int mode, int shift,
                                                     int* __restrict__ hist, int nblk) {
  __shared__ int cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * RT + threadIdx.x;
  if (i < n) atomicAdd(&cnt[digit_of(k, mode, shift, src[i])], 1);
  __syncthreads();
  hist[(long)threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// block-wide exclusive scan of one int per thread (RT threads); *total = sum
__device__ __forceinline__ int block_excl_scan_rt(int v, int* total, int* lds /* >= RT/64 + 1 */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < RT / 64; ++w) { const int t = lds[w]; lds[w] = run; run += t; }
    lds[RT / 64] = run;
  }
  __syncthreads();
  *total = lds[RT / 64];
  return lds[wave] + inc - v;
}

// one workgroup per digit: exclusive scan of its row of tile counts (in place), digit total to tot[d]
__global__ __launch_bounds__(RT) void ev_scan_kernel(int* __restrict__ hist, int nblk, int* __restrict__ tot) {
  __shared__ int lds[RT / 64 + 1];
  int* row = hist + (long)blockIdx.x * nblk;
  int carry = 0;
  for (int b0 = 0; b0 < nblk; b0 += RT) {
    const int b = b0 + threadIdx.x;
    const int v = b < nblk ? row[b] : 0;
    int t;
    const int ex = block_excl_scan_rt(v, &t, lds);
    if (b < nblk) row[b] = carry + ex;
    carry += t;
  }
  if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// stable scatter: tile order, then wave order, then lane order
__global__ __launch_bounds__(RT) void ev_scatter_kernel(const int* __restrict__ src, int* __restrict__ dst, int n, PredKeys k,
                                                        int mode, int shift, const int* __restrict__ hist, int nblk,
                                                        const int* __restrict__ tot) {
  __shared__ int dbase[256];
  __shared__ int wcnt[RT / 64][256];
  __shared__ int lds[RT / 64 + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t;
  dbase[threadIdx.x] = block_excl_scan_rt(tot[threadIdx.x], &t, lds);
  for (int w = 0; w < RT / 64; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * RT + threadIdx.x;
  const bool valid = i < n;
  const int row = valid ? src[i] : 0;
  const unsigned d = valid ? digit_of(k, mode, shift, row) : 0u;
  unsigned long long peers = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < 8; ++bit) {
    const unsigned long long m = __ballot(valid && ((d >> bit) & 1u));
    peers &= ((d >> bit) & 1u) ? m : ~m;
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int my = __popcll(peers & lt);
  if (valid && my == 0) wcnt[wave][d] = __popcll(peers);
  __syncthreads();
  if (valid) {
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wcnt[w][d];
    dst[dbase[d] + hist[(long)d * nblk + blockIdx.x] + before + my] = row;
  }
}

// pos1[perm1[p]] = p, cls1[p] = class key of perm1[p]; the group sort starts from a copy of perm1
__global__ __launch_bounds__(RT) void ev_rank_kernel(const int* __restrict__ perm1, int n, PredKeys k, int* __restrict__ pos1,
                                                     int* __restrict__ cls1, int* __restrict__ copy) {
  const int p = blockIdx.x * RT + threadIdx.x;
  if (p >= n) return;
  const int row = perm1[p];
  pos1[row] = p;
  cls1[p] = cls_key(k, row);
  copy[p] = row;
}

__global__ __launch_bounds__(RT) void ev_key2_kernel(const int* __restrict__ perm2, int n, PredKeys k,
                                                     unsigned long long* __restrict__ key2) {
  const int i = blockIdx.x * RT + threadIdx.x;
  if (i >= n) return;
  const int row = perm2[i];
  key2[i] = ((unsigned long long)cls_key(k, row) << VID_BITS) | (unsigned long long)vid_key(k, row);
}

__global__ __launch_bounds__(RT) void ev_zero_kernel(unsigned char* __restrict__ a, long na, unsigned char* __restrict__ b, long nb) {
  const long i = (long)blockIdx.x * RT + threadIdx.x;
  if (i < na) a[i] = 0;
  if (b && i < nb) b[i] = 0;
}

template <typename T>
__device__ __forceinline__ int lower_bound_dev(const T* a, int n, T key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// tIoU of one prediction against one GT, segment_iou's expression order (metrics.py:357-381).  The ternaries drop a NaN
// prediction boundary where np.maximum / np.minimum keep it, but `pe - ps` carries it into the union: the tIoU is NaN either
// way (tests/test_metrics_edges_gpu.py holds that).
__device__ __forceinline__ double seg_tiou(double ps, double pe, double gs, double ge) {
  const double tt1 = ps > gs ? ps : gs;                  // np.maximum(target[0], candidates[:, 0])
  const double tt2 = pe < ge ? pe : ge;
  double inter = tt2 - tt1;
  if (inter < 0.0) inter = 0.0;                          // .clip(0); NaN stays NaN
  const double uni = (ge - gs) + (pe - ps) - inter;
  return inter / uni;
}

// one wavefront per (class, video) ground-truth group
__global__ __launch_bounds__(64) void ev_match_kernel(const int* __restrict__ perm2, const unsigned long long* __restrict__ key2,
                                                      int n, const int* __restrict__ pos1, const double* __restrict__ ps_,
                                                      const double* __restrict__ pe_, const double* __restrict__ gs_,
                                                      const double* __restrict__ ge_, const int* __restrict__ grp_off,
                                                      const int* __restrict__ grp_cls, const int* __restrict__ grp_vid,
                                                      Thr thr, int n_thr, unsigned* __restrict__ locks,
                                                      unsigned char* __restrict__ tp_rank, unsigned char* __restrict__ tp_out) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int g0 = grp_off[g], g1 = grp_off[g + 1];
  const unsigned long long key = ((unsigned long long)grp_cls[g] << VID_BITS) | (unsigned long long)grp_vid[g];
  const int lo = lower_bound_dev(key2, n, key);
  const int hi = lower_bound_dev(key2, n, key + 1ull);
  for (int j = g0 + lane; j < g1; j += 64) locks[j] = 0u;          // lane-owned: GT j is only ever touched by lane j % 64
  for (int i = lo; i < hi; ++i) {
    const int row = perm2[i];
    const double ps = ps_[row], pe = pe_[row];
    unsigned long long bk[MAX_THR];
    int bj[MAX_THR];
#pragma unroll
    for (int t = 0; t < MAX_THR; ++t) { bk[t] = 0ull; bj[t] = -1; }
    for (int c0 = g0; c0 < g1; c0 += 64) {
      const int j = c0 + lane;
      const bool valid = j < g1;
      double tiou = 0.0;
      unsigned lk = 0u;
      if (valid) { tiou = seg_tiou(ps, pe, gs_[j], ge_[j]); lk = locks[j]; }
      const unsigned long long ok = ord_bits(tiou);              // NaN -> top: argsort()[::-1] visits it first
#pragma unroll
      for (int t = 0; t < MAX_THR; ++t) {
        if (t < n_thr) {
          const bool elig = valid && !(tiou < thr.t[t]) && !((lk >> t) & 1u);
          unsigned long long m = elig ? ok : 0ull;
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
            const unsigned long long v = __shfl_xor(m, o, 64);
            m = v > m ? v : m;
          }
          const unsigned long long who = __ballot(elig && ok == m);
          if (who && m >= bk[t]) {                               // later chunk wins a tie: later GT first
            bk[t] = m;
            bj[t] = c0 + 63 - __clzll(who);
          }
        }
      }
    }
    const int p = pos1[row];
#pragma unroll
    for (int t = 0; t < MAX_THR; ++t) {
      if (t < n_thr && bj[t] >= 0) {
        if (((bj[t] - g0) & 63) == lane) locks[bj[t]] |= 1u << t;
        if (lane == 0) {
          tp_rank[(long)t * n + p] = 1;
          if (tp_out) tp_out[(long)t * n + row] = 1;
        }
      }
    }
  }
}

// one workgroup per (class, threshold); classes are contiguous in rank order (cls1 ascending)
__global__ __launch_bounds__(RT) void ev_ap_kernel(const int* __restrict__ cls1, int n, const unsigned char* __restrict__ tp_rank,
                                                   const int* __restrict__ npos_, int n_cls, double* __restrict__ ap) {
  __shared__ int si[RT];
  __shared__ double sd[RT];
  __shared__ int lds[RT / 64 + 1];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int lo = lower_bound_dev(cls1, n, c), hi = lower_bound_dev(cls1, n, c + 1);
  const int nc = hi - lo;
  if (nc == 0) {
    if (tid == 0) ap[(long)t * n_cls + c] = 0.0;
    return;
  }
  const unsigned char* f = tp_rank + (long)t * n + lo;
  const double npos = (double)npos_[c];
  // pass 1: TP total of the class
  int cnt = 0;
  for (int k = tid; k < nc; k += RT) cnt += f[k];
  int total;
  (void)block_excl_scan_rt(cnt, &total, lds);
  // pass 2: chunks from the end; tp(k) = total - TPs after k; prec(k) = tp / (k + 1) (tp_cumsum + fp_cumsum == k + 1)
  int after = 0;          // TPs in later chunks
  double pmax = 0.0;      // max precision over later chunks (mprec's trailing 0)
  double acc = 0.0;       // this thread's terms, in a fixed order
  const int nchunk = (nc + RT - 1) / RT;
  for (int ch = nchunk - 1; ch >= 0; --ch) {
    const int k = ch * RT + tid;
    const int fl = k < nc ? f[k] : 0;
    // suffix sum of flags inside the chunk (inclusive), via the reversed exclusive scan
    __syncthreads();
    si[RT - 1 - tid] = fl;
    __syncthreads();
    int tch;
    const int rex = block_excl_scan_rt(si[tid], &tch, lds);  // exclusive prefix over reversed order
    __syncthreads();
    si[RT - 1 - tid] = rex;                                  // flags strictly after position tid, inside the chunk
    __syncthreads();
    const int after_me = si[tid];
    const int tp = total - after - after_me;                 // inclusive count at k
    const double prec = k < nc ? (double)tp / (double)(k + 1) : 0.0;
    // suffix max of prec inside the chunk
    sd[tid] = prec;
    __syncthreads();
    for (int o = 1; o < RT; o <<= 1) {
      const double v = tid + o < RT ? sd[tid + o] : 0.0;
      __syncthreads();
      const double cur = sd[tid];
      sd[tid] = v > cur ? v : cur;
      __syncthreads();
    }
    double mp = sd[tid];
    mp = pmax > mp ? pmax : mp;
    if (k < nc && fl) {
      const double rec = (double)tp / npos, rprev = (double)(tp - 1) / npos;
      acc += (rec - rprev) * mp;
    }
    const double m0 = sd[0];
    pmax = pmax > m0 ? pmax : m0;
    after += tch;
  }
  // fixed-order tree over the threads
  __syncthreads();
  sd[tid] = acc;
  __syncthreads();
  for (int o = RT / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  if (tid == 0) ap[(long)t * n_cls + c] = sd[0];
}

// ------------------------------------------------------------------------------------------------------------ Recall@K
// np.maximum / np.minimum and torch.max / torch.min: NaN propagates
__device__ __forceinline__ double nmax(double a, double b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ double nmin(double a, double b) { return (a <= b || a != a) ? a : b; }
__device__ __forceinline__ float nmaxf(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float nminf(float a, float b) { return (a <= b || a != a) ? a : b; }

__global__ __launch_bounds__(64) void ev_hits_zero_kernel(long long* hits, int ncell, long long* total, const int* grp_gt_off,
                                                          int n_grp) {
  for (int i = threadIdx.x; i < ncell; i += 64) hits[i] = 0;
  if (threadIdx.x == 0) *total = grp_gt_off[n_grp];
}

// one wavefront per (video, class name) GT group; predictions of the group in result order
__global__ __launch_bounds__(64) void ev_hits_kernel(const double* __restrict__ ps_, const double* __restrict__ pe_,
                                                     const int* __restrict__ grp_pred_off, const int* __restrict__ grp_pred_cnt,
                                                     const double* __restrict__ gs_, const double* __restrict__ ge_,
                                                     const int* __restrict__ grp_gt_off, Thr thr, int n_thr, Ranks rk,
                                                     int n_rank, long long* __restrict__ hits) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const int g0 = grp_gt_off[g], g1 = grp_gt_off[g + 1];
  const int ngt = g1 - g0;
  const int p0 = grp_pred_off[g], np = grp_pred_cnt[g];
  int rmax = 0;
  for (int r = 0; r < n_rank; ++r) rmax = rk.r[r] > rmax ? rk.r[r] : rmax;
  const long lim = (long)rmax * ngt;
  const int m = (int)(np < lim ? np : lim);
  for (int c0 = g0; c0 < g1; c0 += 64) {
    const int j = c0 + lane;
    const bool valid = j < g1;
    const double gs = valid ? gs_[j] : 0.0, ge = valid ? ge_[j] : 0.0;
    unsigned hit[MAX_RANK];                                    // bit t: retrieved at threshold t within rank r
#pragma unroll
    for (int r = 0; r < MAX_RANK; ++r) hit[r] = 0u;
    if (valid) {
      for (int i = 0; i < m; ++i) {
        const double ps = ps_[p0 + i], pe = pe_[p0 + i];
        // iou() (get_retrieval_performance.py:166-184): a NaN boundary on either side gives a NaN overlap, no hit
        const double inter = nmax(0.0, nmin(pe, ge) - nmax(ps, gs));
        const double uni = nmax(0.0, nmax(pe, ge) - nmin(ps, gs));
        const double ov = 1.0 * inter / uni;
        unsigned bits = 0u;
        for (int t = 0; t < n_thr; ++t) bits |= (ov > thr.t[t]) ? (1u << t) : 0u;
#pragma unroll
        for (int r = 0; r < MAX_RANK; ++r)
          if (r < n_rank && (long)i < (long)rk.r[r] * ngt) hit[r] |= bits;
      }
    }
    for (int t = 0; t < n_thr; ++t)
      for (int r = 0; r < n_rank; ++r) {
        const int cnt = __popcll(__ballot(valid && ((hit[r] >> t) & 1u)));
        if (lane == 0 && cnt) atomicAdd((unsigned long long*)&hits[t * n_rank + r], (unsigned long long)cnt);
      }
  }
}

// ------------------------------------------------------------------------------------------------ NLQ Recall@K and mIoU
// NLQ/libs/utils/metrics.py ReferringRecall: one ground-truth window per query, the query's predictions in result order.
//   mode 0  compute_IoU (:47-68, NumPy, fp64): intersection and hull both clamped at 0, overlap = 1.0 * inter / union
//   mode 1  _iou (:142-147, torch, fp32): operands rounded to fp32, intersection clamped, hull not, fp32 quotient widened
// query kernel    one lane per query: IoU of its first min(cnt, max K) rows, top1[q], one 16-bit word of threshold bits per
//                 (rank, query) into the workspace, optionally the flags [q][t][r]
// segment kernel  one workgroup per segment: integer sums of the words' bits, the query count and the sum of top1, each
//                 thread over its queries in index order, then a fixed tree -- no atomics, repeated calls are bit-equal.
//                 It reads n_seg * n_query segment ids; n_seg is the number of query templates (13 in the benchmark).
enum { NLQ_NUMPY64 = 0, NLQ_TORCH32 = 1 };

__device__ __forceinline__ double nlq_iou64(double ps, double pe, double gs, double ge) {
  const double inter = nmax(0.0, nmin(pe, ge) - nmax(ps, gs));
  const double uni = nmax(0.0, nmax(pe, ge) - nmin(ps, gs));
  return 1.0 * inter / uni;
}

__device__ __forceinline__ double nlq_iou32(float ps, float pe, float gs, float ge) {
  const float inter = nminf(pe, ge) - nmaxf(ps, gs);
  const float uni = nmaxf(pe, ge) - nminf(ps, gs);
  const float cl = (inter < 0.0f) ? 0.0f : inter;              // clamp(min=0); NaN stays NaN
  // the fp32 quotient, correctly rounded: 53 >= 2 * 24 + 2 bits, so rounding the fp64 quotient again is exact rounding
  const float q = (float)((double)cl / (double)uni);
  return (double)q;
}

template <typename T2>
__global__ __launch_bounds__(RT) void ev_nlq_query_kernel(const T2* __restrict__ pred, const int* __restrict__ pred_cnt,
                                                          int k_cap, const double2* __restrict__ gt, int n, Thr thr, int n_thr,
                                                          Ranks rk, int n_rank, int mode, double* __restrict__ top1,
                                                          unsigned short* __restrict__ words,
                                                          unsigned char* __restrict__ flags) {
  const int q = blockIdx.x * RT + threadIdx.x;
  if (q >= n) return;
  int rmax = 1;
  for (int r = 0; r < n_rank; ++r) rmax = rk.r[r] > rmax ? rk.r[r] : rmax;
  int cnt = pred_cnt[q];
  cnt = cnt < 0 ? 0 : (cnt > k_cap ? k_cap : cnt);              // rows past the count (and past k_cap) are never read
  const int m = cnt < rmax ? cnt : rmax;
  const double2 g = gt[q];
  const float gsf = (float)g.x, gef = (float)g.y;
  const T2* rows = pred + (long)q * k_cap;
  unsigned hit[MAX_RANK];                                       // bit t: one of the first K rows has IoU > threshold t
#pragma unroll
  for (int r = 0; r < MAX_RANK; ++r) hit[r] = 0u;
  double first = __longlong_as_double(0x7ff8000000000000ll);    // a query without rows has no first IoU
  for (int i = 0; i < m; ++i) {
    const T2 p = rows[i];
    const double ov = mode == NLQ_TORCH32 ? nlq_iou32((float)p.x, (float)p.y, gsf, gef)
                                          : nlq_iou64((double)p.x, (double)p.y, g.x, g.y);
    if (i == 0) first = ov;
    unsigned bits = 0u;
    for (int t = 0; t < n_thr; ++t) bits |= (ov > thr.t[t]) ? (1u << t) : 0u;
#pragma unroll
    for (int r = 0; r < MAX_RANK; ++r)
      if (r < n_rank && i < rk.r[r]) hit[r] |= bits;
  }
  top1[q] = first;
#pragma unroll
  for (int r = 0; r < MAX_RANK; ++r)
    if (r < n_rank) {
      words[(long)r * n + q] = (unsigned short)hit[r];
      if (flags)
        for (int t = 0; t < n_thr; ++t) flags[((long)q * n_thr + t) * n_rank + r] = (unsigned char)((hit[r] >> t) & 1u);
    }
}

// block-wide integer sum (RT threads); every thread gets the total
__device__ __forceinline__ long long block_sum_rt(long long v, long long* lds /* >= RT/64 */) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  long long s = 0;
  for (int w = 0; w < RT / 64; ++w) s += lds[w];
  return s;
}

__global__ __launch_bounds__(RT) void ev_nlq_segment_kernel(const unsigned short* __restrict__ words,
                                                            const double* __restrict__ top1, const int* __restrict__ seg_id,
                                                            int n, int n_thr, int n_rank, long long* __restrict__ hits,
                                                            long long* __restrict__ n_out, double* __restrict__ sum_out) {
  __shared__ long long li[RT / 64];
  __shared__ double sd[RT];
  const int s = blockIdx.x, tid = threadIdx.x;
  for (int r = 0; r < n_rank; ++r) {
    int c[MAX_THR];
#pragma unroll
    for (int t = 0; t < MAX_THR; ++t) c[t] = 0;
    for (int q = tid; q < n; q += RT) {
      if ((seg_id ? seg_id[q] : 0) != s) continue;              // ids outside [0, n_seg) belong to no segment
      const unsigned w = words[(long)r * n + q];
#pragma unroll
      for (int t = 0; t < MAX_THR; ++t) c[t] += (int)((w >> t) & 1u);
    }
#pragma unroll
    for (int t = 0; t < MAX_THR; ++t)
      if (t < n_thr) {
        const long long tot = block_sum_rt((long long)c[t], li);
        if (tid == 0) hits[((long)s * n_thr + t) * n_rank + r] = tot;
      }
  }
  int cnt = 0;
  double acc = 0.0;
  for (int q = tid; q < n; q += RT)
    if ((seg_id ? seg_id[q] : 0) == s) { ++cnt; acc += top1[q]; }
  const long long tot = block_sum_rt((long long)cnt, li);
  sd[tid] = acc;
  __syncthreads();
  for (int o = RT / 2; o >= 1; o >>= 1) {
    if (tid < o) sd[tid] = sd[tid] + sd[tid + o];
    __syncthreads();
  }
  if (tid == 0) { n_out[s] = tot; sum_out[s] = sd[0]; }
}

struct DetWs {
  int *a, *b, *c, *pos1, *cls1, *hist, *tot;
  unsigned long long* key2;
  unsigned* locks;
  unsigned char* tp_rank;
  size_t bytes;
};

size_t al256(size_t x) { return (x + 255) / 256 * 256; }

DetWs det_ws_layout(char* base, long n, int n_gt, int n_thr) {
  const long nn = n > 0 ? n : 1;
  const long nblk = (nn + RT - 1) / RT;
  DetWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base + off; off += al256(bytes); return p; };
  w.a = (int*)take(nn * 4); w.b = (int*)take(nn * 4); w.c = (int*)take(nn * 4);
  w.pos1 = (int*)take(nn * 4); w.cls1 = (int*)take(nn * 4);
  w.hist = (int*)take((size_t)256 * nblk * 4); w.tot = (int*)take(256 * 4);
  w.key2 = (unsigned long long*)take(nn * 8);
  w.locks = (unsigned*)take((size_t)(n_gt > 0 ? n_gt : 1) * 4);
  w.tp_rank = (unsigned char*)take((size_t)nn * (n_thr > 0 ? n_thr : 1));
  w.bytes = off;
  return w;
}

int key_passes(long range) {          // 8-bit passes for keys 0..range
  int p = 0;
  while (range > 0) { ++p; range >>= 8; }
  return p > 0 ? p : 1;
}

// stable LSD passes over one key; the result ends in *src (ping-pong with *tmp)
void sort_by(int** src, int** tmp, int n, const PredKeys& k, int mode, int passes, int* hist, int* tot, hipStream_t s) {
  const int nblk = (n + RT - 1) / RT;
  for (int p = 0; p < passes; ++p) {
    hipLaunchKernelGGL(ev_hist_kernel, dim3(nblk), dim3(RT), 0, s, *src, n, k, mode, 8 * p, hist, nblk);
    hipLaunchKernelGGL(ev_scan_kernel, dim3(256), dim3(RT), 0, s, hist, nblk, tot);
    hipLaunchKernelGGL(ev_scatter_kernel, dim3(nblk), dim3(RT), 0, s, *src, *tmp, n, k, mode, 8 * p, hist, nblk, tot);
    int* x = *src; *src = *tmp; *tmp = x;
  }
}

}  // namespace

extern "C" size_t vilco_det_ap_workspace(int64_t n_pred, int32_t n_gt, int32_t n_thr) {
  if (n_pred < 0 || n_gt < 0 || n_thr < 0 || n_pred > 0x7ffffffeL) return 0;
  return det_ws_layout(nullptr, (long)n_pred, n_gt, n_thr).bytes + 256;
}

extern "C" int vilco_det_ap(const int32_t* pred_vid, const int32_t* pred_cls, const double* pred_start, const double* pred_end,
                            const double* pred_score, int64_t n_pred, const double* gt_start, const double* gt_end,
                            const int32_t* grp_off, const int32_t* grp_cls, const int32_t* grp_vid, int32_t n_grp, int32_t n_gt,
                            const int32_t* cls_npos, int32_t n_cls, int32_t n_vid, const double* thresholds, int32_t n_thr,
                            double* ap, uint8_t* tp_flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_pred < 0 || n_grp < 0 || n_gt < 0 || n_cls < 0 || n_vid < 0 || n_thr < 0) return VILCO_ERR_BADARG;
  if (!thresholds || !ap || !cls_npos || !grp_off || !workspace) return VILCO_ERR_BADARG;
  if (n_pred > 0 && (!pred_vid || !pred_cls || !pred_start || !pred_end || !pred_score)) return VILCO_ERR_BADARG;
  if (n_grp > 0 && (!grp_cls || !grp_vid || !gt_start || !gt_end)) return VILCO_ERR_BADARG;
  if (n_thr < 1 || n_thr > MAX_THR) return VILCO_ERR_UNSUPPORTED;
  if (n_cls >= (1 << 16) || n_vid >= (1 << VID_BITS) - 1 || n_pred > 0x7ffffffeL) return VILCO_ERR_UNSUPPORTED;
  if (workspace_bytes < vilco_det_ap_workspace(n_pred, n_gt, n_thr)) return VILCO_ERR_WORKSPACE;
  if (n_cls == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  const int n = (int)n_pred;
  DetWs w = det_ws_layout(base, n, n_gt, n_thr);
  Thr thr{};
  for (int t = 0; t < n_thr; ++t) thr.t[t] = thresholds[t];
  const int nblk = (n + RT - 1) / RT;
  if (n > 0) {
    PredKeys k{pred_vid, pred_cls, pred_score, n_cls, n_vid};
    const int cls_p = key_passes(n_cls), vid_p = key_passes(n_vid);
    int *src = w.a, *tmp = w.b;
    hipLaunchKernelGGL(ev_iota_rev_kernel, dim3(nblk), dim3(RT), 0, s, src, n);
    sort_by(&src, &tmp, n, k, KEY_SCORE, 8, w.hist, w.tot, s);
    sort_by(&src, &tmp, n, k, KEY_CLS, cls_p, w.hist, w.tot, s);
    int* perm1 = src;
    int* g_src = tmp;
    int* g_tmp = w.c;
    hipLaunchKernelGGL(ev_rank_kernel, dim3(nblk), dim3(RT), 0, s, perm1, n, k, w.pos1, w.cls1, g_src);
    sort_by(&g_src, &g_tmp, n, k, KEY_VID, vid_p, w.hist, w.tot, s);
    sort_by(&g_src, &g_tmp, n, k, KEY_CLS, cls_p, w.hist, w.tot, s);
    hipLaunchKernelGGL(ev_key2_kernel, dim3(nblk), dim3(RT), 0, s, g_src, n, k, w.key2);
    const long nz = (long)n * n_thr;
    hipLaunchKernelGGL(ev_zero_kernel, dim3((unsigned)((nz + RT - 1) / RT)), dim3(RT), 0, s, w.tp_rank, nz, tp_flags, nz);
    if (n_grp > 0)
      hipLaunchKernelGGL(ev_match_kernel, dim3(n_grp), dim3(64), 0, s, g_src, w.key2, n, w.pos1, pred_start, pred_end, gt_start,
                         gt_end, grp_off, grp_cls, grp_vid, thr, (int)n_thr, w.locks, w.tp_rank, tp_flags);
  }
  hipLaunchKernelGGL(ev_ap_kernel, dim3(n_cls, n_thr), dim3(RT), 0, s, w.cls1, n, w.tp_rank, cls_npos, (int)n_cls, ap);
  return vilco_launch_status();
}

extern "C" size_t vilco_retrieval_hits_workspace(int32_t n_grp, int32_t n_thr, int32_t n_rank) {
  (void)n_grp; (void)n_thr; (void)n_rank;
  return 0;       // the hit counts are integer sums straight into the output
}

extern "C" int vilco_retrieval_hits(const double* pred_start, const double* pred_end, const int32_t* grp_pred_off,
                                    const int32_t* grp_pred_cnt, const double* gt_start, const double* gt_end,
                                    const int32_t* grp_gt_off, int32_t n_grp, const double* thresholds, int32_t n_thr,
                                    const int32_t* ranks, int32_t n_rank, int64_t* hits, int64_t* total, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (n_grp < 0 || n_thr < 0 || n_rank < 0) return VILCO_ERR_BADARG;
  if (!thresholds || !ranks || !hits || !total || !grp_gt_off) return VILCO_ERR_BADARG;
  if (n_grp > 0 && (!grp_pred_off || !grp_pred_cnt || !gt_start || !gt_end || !pred_start || !pred_end))
    return VILCO_ERR_BADARG;
  if (n_thr < 1 || n_thr > MAX_THR || n_rank < 1 || n_rank > MAX_RANK) return VILCO_ERR_UNSUPPORTED;
  for (int r = 0; r < n_rank; ++r)
    if (ranks[r] < 0) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_retrieval_hits_workspace(n_grp, n_thr, n_rank)) return VILCO_ERR_WORKSPACE;
  (void)workspace;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Thr thr{};
  Ranks rk{};
  for (int t = 0; t < n_thr; ++t) thr.t[t] = thresholds[t];
  for (int r = 0; r < n_rank; ++r) rk.r[r] = ranks[r];
  long long* h = reinterpret_cast<long long*>(hits);
  hipLaunchKernelGGL(ev_hits_zero_kernel, dim3(1), dim3(64), 0, s, h, (int)(n_thr * n_rank), reinterpret_cast<long long*>(total),
                     grp_gt_off, (int)n_grp);
  if (n_grp > 0)
    hipLaunchKernelGGL(ev_hits_kernel, dim3(n_grp), dim3(64), 0, s, pred_start, pred_end, grp_pred_off, grp_pred_cnt, gt_start,
                       gt_end, grp_gt_off, thr, (int)n_thr, rk, (int)n_rank, h);
  return vilco_launch_status();
}

extern "C" size_t vilco_nlq_recall_workspace(int64_t n_query, int32_t n_rank) {
  if (n_query < 0 || n_query > 0x7ffffffeL || n_rank < 1 || n_rank > MAX_RANK) return 0;
  return al256((size_t)(n_query > 0 ? n_query : 1) * n_rank * sizeof(unsigned short)) + 256;
}

extern "C" int vilco_nlq_recall(const void* pred, int32_t pred_fp32, const int32_t* pred_cnt, int32_t k_cap, const double* gt,
                                const int32_t* seg_id, int64_t n_query, int32_t n_seg, const double* thresholds, int32_t n_thr,
                                const int32_t* ranks, int32_t n_rank, int32_t mode, int64_t* hits, int64_t* n, double* top1,
                                double* top1_sum, uint8_t* flags, void* workspace, size_t workspace_bytes, void* stream) {
  if (n_query < 0 || n_seg < 1 || n_thr < 0 || n_rank < 0 || k_cap < 1) return VILCO_ERR_BADARG;
  if (!thresholds || !ranks || !hits || !n || !top1 || !top1_sum || !workspace) return VILCO_ERR_BADARG;
  if (n_query > 0 && (!pred || !pred_cnt || !gt)) return VILCO_ERR_BADARG;
  if (reinterpret_cast<uintptr_t>(gt) % 16 || reinterpret_cast<uintptr_t>(pred) % (pred_fp32 ? 8 : 16))
    return VILCO_ERR_BADARG;                                   // rows are read as whole vectors
  if (n_thr < 1 || n_thr > MAX_THR || n_rank < 1 || n_rank > MAX_RANK || n_query > 0x7ffffffeL) return VILCO_ERR_UNSUPPORTED;
  if (mode != NLQ_NUMPY64 && mode != NLQ_TORCH32) return VILCO_ERR_UNSUPPORTED;
  for (int r = 0; r < n_rank; ++r)
    if (ranks[r] < 1) return VILCO_ERR_BADARG;
  if (workspace_bytes < vilco_nlq_recall_workspace(n_query, n_rank)) return VILCO_ERR_WORKSPACE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned short* words = reinterpret_cast<unsigned short*>((reinterpret_cast<uintptr_t>(workspace) + 255) / 256 * 256);
  Thr thr{};
  Ranks rk{};
  for (int t = 0; t < n_thr; ++t) thr.t[t] = thresholds[t];
  for (int r = 0; r < n_rank; ++r) rk.r[r] = ranks[r];
  const int nq = (int)n_query;
  if (nq > 0) {
    const dim3 grid((unsigned)((nq + RT - 1) / RT));
    const double2* g2 = reinterpret_cast<const double2*>(gt);
    if (pred_fp32)
      hipLaunchKernelGGL(ev_nlq_query_kernel<float2>, grid, dim3(RT), 0, s, reinterpret_cast<const float2*>(pred), pred_cnt,
                         (int)k_cap, g2, nq, thr, (int)n_thr, rk, (int)n_rank, (int)mode, top1, words, flags);
    else
      hipLaunchKernelGGL(ev_nlq_query_kernel<double2>, grid, dim3(RT), 0, s, reinterpret_cast<const double2*>(pred), pred_cnt,
                         (int)k_cap, g2, nq, thr, (int)n_thr, rk, (int)n_rank, (int)mode, top1, words, flags);
  }
  hipLaunchKernelGGL(ev_nlq_segment_kernel, dim3(n_seg), dim3(RT), 0, s, words, top1, seg_id, nq, (int)n_thr, (int)n_rank,
                     reinterpret_cast<long long*>(hits), reinterpret_cast<long long*>(n), top1_sum);
  return vilco_launch_status();
}
