// Step glue of the training loop (MQ/libs/utils/train_utils.py:343-351): global-L2-norm gradient clipping
// (torch.nn.utils.clip_grad_norm_) and the AdamW / SGD-momentum update of torch.optim, as multi-tensor kernels:
// ONE launch walks every parameter tensor through a chunk table, so the 358 gradient-bearing tensors of config P
// (210.7 M parameters, 28 B/param of HBM traffic for AdamW) cost 3 launches instead of ~1500.
// The clip coefficient stays on the device (no host sync) and is applied to the gradient inside the update.
#include "common.h"

namespace {

constexpr int OPT_THREADS = 256;

// the device's copy of a vilco_chunk_table (layout: include/vilco_hip.h), made by table_args() below
struct MultiArgs {
  const long* ptrs;          // [rows][n] device pointers
  const long* numel;         // [n]
  const int* chunk_tensor;   // [nchunks]
  const long* chunk_off;     // [nchunks] element offset inside the tensor
  const int* group;          // [n] parameter-group index (the optimizer's; null elsewhere)
  int n, chunk;
};

// What block blockIdx.x walks: elements off .. off + cnt of tensor t, row<T>(k) = where they start in row k.  A chunk that lies
// outside its tensor gets cnt = 0 and no early return: a kernel that owes a per-chunk partial still writes it.
struct ChunkView {
  const long* col;           // &ptrs[0][t]
  long n;
  int t;
  long off, cnt;
  template <typename T>
  __device__ __forceinline__ T* row(int k) const { return reinterpret_cast<T*>(col[k * n]) + off; }
};

__device__ __forceinline__ ChunkView chunk_view(const MultiArgs& a) {
  const int t = a.chunk_tensor[blockIdx.x];
  const long off = a.chunk_off[blockIdx.x];
  long cnt = a.numel[t] - off;
  if (cnt > a.chunk) cnt = a.chunk;
  if (off < 0 || cnt < 0) cnt = 0;
  return ChunkView{a.ptrs + t, (long)a.n, t, off, cnt};
}

// *dst = the block's sum of s: wave sums, then (r0 + r1) + (r2 + r3)
__device__ __forceinline__ void block_sum_to(float s, float* __restrict__ dst) {
  __shared__ float red[OPT_THREADS / 64];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (red[0] + red[1]) + (red[2] + red[3]);
}

// sum of partial[0..n) in double over ONE block of OPT_THREADS threads: strided per-thread sums, then a halving tree
__device__ __forceinline__ double partials_sum(const float* __restrict__ partial, int n) {
  __shared__ double red[OPT_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += OPT_THREADS) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(OPT_THREADS) void sqnorm_kernel(MultiArgs a, float* __restrict__ partial) {
  const ChunkView c = chunk_view(a);
  const float* g = c.row<const float>(1);
  float s = 0.f;
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) s += g[i] * g[i];
  block_sum_to(s, partial + blockIdx.x);
}

// out[0] = total L2 norm, out[1] = clip coefficient min(1, max_norm / (norm + 1e-6))   (max_norm <= 0: coef 1)
__global__ __launch_bounds__(OPT_THREADS) void clip_coef_kernel(const float* __restrict__ partial, int n,
                                                                float max_norm, float* __restrict__ out) {
  const double total = partials_sum(partial, n);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    out[0] = norm;
    float c = 1.f;
    if (max_norm > 0.f) {
      c = max_norm / (norm + 1e-6f);
      if (c > 1.f) c = 1.f;
    }
    out[1] = c;
  }
}

// out[0] = scale * sum of the partials
__global__ __launch_bounds__(OPT_THREADS) void scaled_sum_kernel(const float* __restrict__ partial, int n, float scale,
                                                                 float* __restrict__ out) {
  const double total = partials_sum(partial, n);
  if (threadIdx.x == 0) out[0] = (float)(total * (double)scale);
}

struct Hyper {
  float lr[8], wd[8];
  float beta1, beta2, eps;
  float log_beta1, log_beta2;              // log(beta), taken in double on the host: 1 - beta^t = -expm1f(t log beta)
  float momentum;                          // SGD
  const float* tstep;                      // [n] per-tensor step count (after this update), torch keeps it per param;
                                           // SGD only asks whether it is <= 1 (the momentum buffer starts as the gradient)
  const float* lr_dev;                     // optional [ngroups] learning rates in device memory (override lr[]): a captured
                                           // step replays its kernel arguments, the schedule's value must come from memory
};

// torch.optim.AdamW (decoupled weight decay): p *= 1 - lr*wd ; m,v EMA ; p -= lr/bias1 * m / (sqrt(v)/sqrt(bias2) + eps)
// chunk_amax (optional): max|p| of the UPDATED parameter over each chunk -- the optimizer is the producer of next step's
// weights, so the fp16 x2 weight packs take their per-tensor scale from these partials instead of re-reading the weight
__device__ __forceinline__ void emit_chunk_amax(float mx, float* __restrict__ chunk_amax) {
  __shared__ float red[OPT_THREADS / 64];
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) chunk_amax[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// SI (Synaptic Intelligence, Zenke et al. 2017): the update also advances the path integral of every regularised
// tensor, omega <- fmaf(-gr, p_new - p_old, omega), gr = the clipped gradient the update consumes, p_new - p_old the fp32
// difference of the stored values (so it contains the weight decay).  si_ptrs [n] = address of each tensor's omega (the
// parameter's element count, walked with the same chunk table), 0 = not regularised.  Old value, gradient and new value are in
// registers here: the cost is one more read-modify-write stream, no launch, no atomics (every element has one owner thread).
// SI = false never reads si_ptrs and is the kernel as it was.
// RWalk (Riemannian Walk; Chaudhry, Dokania, Ajanthan, Torr, ECCV 2018): besides SI's path integral w (si_ptrs is its
// table) the update keeps an exponential moving average of the squared gradient, the diagonal empirical Fisher F, and every
// delta_t iterations closes the interval: the path score s gains max(w, 0) / (0.5 F d^2 + eps), d = p_new - theta_ck.
// rw_ptrs [3][n] = addresses of fisher, score, theta_ck; tick = ONE device word, the iterations since the task began counted
// after this one -- read from memory, so a replayed launch follows it.  The checkpoint branch is uniform over the grid; score and
// theta_ck are neither loaded nor stored outside it.
struct RwalkArgs {
  const long* rw_ptrs;
  const int* tick;
  float alpha, eps;
  int delta_t;
};

// what a tracked element keeps besides the optimizer state: TRACK 1 = SI (om), 2 = RWalk (all four)
struct TrackPtrs {
  float *om, *fi, *sc, *ck;
  bool ckpt;
};

template <int TRACK>
__device__ __forceinline__ TrackPtrs track_ptrs(const ChunkView& cv, const long* __restrict__ si_ptrs, const RwalkArgs& rw) {
  TrackPtrs tp{nullptr, nullptr, nullptr, nullptr, false};
  if constexpr (TRACK != 0) {
    const long oa = si_ptrs[cv.t];
    if (oa) tp.om = reinterpret_cast<float*>(oa) + cv.off;
  }
  if constexpr (TRACK == 2) {
    if (tp.om) {
      tp.fi = reinterpret_cast<float*>(rw.rw_ptrs[cv.t]) + cv.off;
      tp.sc = reinterpret_cast<float*>(rw.rw_ptrs[cv.n + cv.t]) + cv.off;
      tp.ck = reinterpret_cast<float*>(rw.rw_ptrs[2 * cv.n + cv.t]) + cv.off;
    }
    tp.ckpt = (*rw.tick % rw.delta_t) == 0;
  }
  return tp;
}

// RWalk's share of one element's update, after p_new is known.  fn = F + alpha (gr gr - F): four roundings, in this order (the
// callers hold fp contract off).  The score's quotient and sum are formed in double and rounded once, as si_consolidate_kernel.
__device__ __forceinline__ void rwalk_element(const TrackPtrs& tp, const RwalkArgs& rw, long i, float gr, float p0, float pv,
                                              float ov, float fv, float sv, float kv) {
#pragma clang fp contract(off)
  const float fn = fv + rw.alpha * (gr * gr - fv);
  const float wn = __fmaf_rn(-gr, pv - p0, ov);
  tp.fi[i] = fn;
  if (tp.ckpt) {
    const double d = (double)pv - (double)kv;
    const double q = (double)fmaxf(wn, 0.f) / (0.5 * (double)fn * d * d + (double)rw.eps);
    tp.sc[i] = (float)((double)sv + q);
    tp.om[i] = 0.f;
    tp.ck[i] = pv;
  } else {
    tp.om[i] = wn;
  }
}

template <int TRACK>
__device__ __forceinline__ void adamw_body(const MultiArgs& a, const Hyper& h, const float* __restrict__ coef,
                                           float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs, const RwalkArgs& rw) {
  const ChunkView cv = chunk_view(a);
  const int t = cv.t;
  const long cnt = cv.cnt;
  float* p = cv.row<float>(0);
  const float* g = cv.row<const float>(1);
  float* m = cv.row<float>(2);
  float* v = cv.row<float>(3);
  const int gi = a.group[t];
  const float lr = h.lr_dev ? h.lr_dev[gi] : h.lr[gi], wd = h.wd[gi];
  const float c = coef ? coef[1] : 1.f;
  const float stp = h.tstep[t];
  // bias corrections 1 - beta^step: as 1.f - powf(beta, step) the subtraction cancels for small step counts (beta2 = 0.999:
  // ~100 roundings at steps 2..5), and half of that reaches the update through the square root
  const float step_size = lr / -expm1f(stp * h.log_beta1);
  const float rs2 = sqrtf(-expm1f(stp * h.log_beta2));
  const TrackPtrs tp = track_ptrs<TRACK>(cv, si_ptrs, rw);
  float* om = tp.om;
  float mx = 0.f;
  for (long i = threadIdx.x; i < cnt; i += OPT_THREADS) {
    const float keep = 1.f - lr * wd;
    {
      // every product and sum of the element's update is rounded on its own: that is how this loop has always been compiled
      // (packed multiplies, no fused multiply-add), and the pragma holds every instantiation to it -- the path integral's and
      // RWalk's extra uses of gr and pv must not change a bit of p, m or v
#pragma clang fp contract(off)
      const float gr = g[i] * c;
      const float p0 = p[i];
      float ov = 0.f, fv = 0.f, sv = 0.f, kv = 0.f;
      if constexpr (TRACK != 0) {
        if (om) ov = om[i];          // issued with the other loads, not behind the stores
      }
      if constexpr (TRACK == 2) {
        if (om) {
          fv = tp.fi[i];
          if (tp.ckpt) { sv = tp.sc[i]; kv = tp.ck[i]; }
        }
      }
      float pv = p0 * keep;
      const float mv = h.beta1 * m[i] + (1.f - h.beta1) * gr;
      const float vv = h.beta2 * v[i] + (1.f - h.beta2) * gr * gr;
      m[i] = mv;
      v[i] = vv;
      pv -= step_size * (mv / (sqrtf(vv) / rs2 + h.eps));
      p[i] = pv;
      if constexpr (TRACK == 1) {
        if (om) om[i] = __fmaf_rn(-gr, pv - p0, ov);
      }
      if constexpr (TRACK == 2) {
        if (om) rwalk_element(tp, rw, i, gr, p0, pv, ov, fv, sv, kv);
      }
      mx = fmaxf(mx, fabsf(pv));
    }
  }
  if (chunk_amax) emit_chunk_amax(mx, chunk_amax);
}

template <bool SI>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(MultiArgs a, Hyper h, const float* __restrict__ coef,
                                                            float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs) {
  adamw_body<SI ? 1 : 0>(a, h, coef, chunk_amax, si_ptrs, RwalkArgs{});
}

__global__ __launch_bounds__(OPT_THREADS) void adamw_rwalk_kernel(MultiArgs a, Hyper h, const float* __restrict__ coef,
                                                                  float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs,
                                                                  RwalkArgs rw) {
  adamw_body<2>(a, h, coef, chunk_amax, si_ptrs, rw);
}

// torch.optim.SGD with momentum (no dampening / nesterov): g += wd*p ; buf = first ? g : mom*buf + g ; p -= lr*buf
// SI: as in adamw_kernel; gr is the clipped gradient BEFORE wd * p is added to it
template <int TRACK>
__device__ __forceinline__ void sgd_body(const MultiArgs& a, const Hyper& h, const float* __restrict__ coef,
                                         float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs, const RwalkArgs& rw) {
  const ChunkView cv = chunk_view(a);
  const int t = cv.t;
  const long cnt = cv.cnt;
  float* p = cv.row<float>(0);
  const float* g = cv.row<const float>(1);
  float* m = cv.row<float>(2);
  const int gi = a.group[t];
  const float lr = h.lr_dev ? h.lr_dev[gi] : h.lr[gi], wd = h.wd[gi];
  const float c = coef ? coef[1] : 1.f;
  const bool first = h.tstep[t] <= 1.f;          // momentum buffer starts as the first gradient
  const TrackPtrs tp = track_ptrs<TRACK>(cv, si_ptrs, rw);
  float* om = tp.om;
  float mx = 0.f;
  for (long i = threadIdx.x; i < cnt; i += OPT_THREADS) {
    // the roundings this loop has always been compiled to, spelled out so that every instantiation keeps them whatever else uses
    // gc and pv: c g and wd p rounded on their own and added; momentum buf + d and p - lr buf fused
#pragma clang fp contract(off)
    const float pv0 = p[i];
    const float gc = g[i] * c;
    float ov = 0.f, fv = 0.f, sv = 0.f, kv = 0.f;
    if constexpr (TRACK != 0) {
      if (om) ov = om[i];
    }
    if constexpr (TRACK == 2) {
      if (om) {
        fv = tp.fi[i];
        if (tp.ckpt) { sv = tp.sc[i]; kv = tp.ck[i]; }
      }
    }
    float gr = gc + wd * pv0;
    const float b = first ? gr : __fmaf_rn(h.momentum, m[i], gr);
    m[i] = b;
    const float pv = __fmaf_rn(-lr, b, pv0);
    p[i] = pv;
    if constexpr (TRACK == 1) {
      if (om) om[i] = __fmaf_rn(-gc, pv - pv0, ov);
    }
    if constexpr (TRACK == 2) {
      if (om) rwalk_element(tp, rw, i, gc, pv0, pv, ov, fv, sv, kv);
    }
    mx = fmaxf(mx, fabsf(pv));
  }
  if (chunk_amax) emit_chunk_amax(mx, chunk_amax);
}

template <bool SI>
__global__ __launch_bounds__(OPT_THREADS) void sgd_kernel(MultiArgs a, Hyper h, const float* __restrict__ coef,
                                                          float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs) {
  sgd_body<SI ? 1 : 0>(a, h, coef, chunk_amax, si_ptrs, RwalkArgs{});
}

__global__ __launch_bounds__(OPT_THREADS) void sgd_rwalk_kernel(MultiArgs a, Hyper h, const float* __restrict__ coef,
                                                                float* __restrict__ chunk_amax, const long* __restrict__ si_ptrs,
                                                                RwalkArgs rw) {
  sgd_body<2>(a, h, coef, chunk_amax, si_ptrs, rw);
}

// EWC / MAS penalty (MQ/libs/cl_methods/EWC.py:6-22, MAS.py:5-21) over a chunk table of (parameter, importance,
// consolidated value) triples: partial[chunk] = sum F (opt - p)^2 ; grad += -2 lambda F (opt - p).
// The added term is formed in double and rounded once (the kernels are bound by their five streams, not by arithmetic), so an
// element's gradient carries one rounding per add and one for the term: independent of the order atomics arrive in.
// rows: param, grad, importance, optpar; numel[t] = optpar's element count (a prefix of the parameter when the class head has
// grown).  ATOMIC: a parameter appears in more than one task's dictionary, so its gradient is accumulated with atomics.
template <bool ATOMIC>
__global__ __launch_bounds__(OPT_THREADS) void cl_penalty_kernel(MultiArgs a, float lambda, float* __restrict__ partial) {
  const ChunkView c = chunk_view(a);
  const float* p = c.row<const float>(0);
  float* g = c.row<float>(1);
  const float* f = c.row<const float>(2);
  const float* o = c.row<const float>(3);
  float s = 0.f;
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) {
    const double d = (double)o[i] - (double)p[i];
    const double fd = (double)f[i] * d;
    s += (float)(fd * d);
    if constexpr (ATOMIC) atomicAdd(&g[i], (float)(-2.0 * (double)lambda * fd));
    else g[i] = (float)((double)g[i] - 2.0 * (double)lambda * fd);      // every parameter occurs once: plain read-modify-write
  }
  block_sum_to(s, partial + blockIdx.x);
}

// Importance accumulation of the consolidation pass (MQ/libs/cl_methods/EWC.py:24-56, MAS.py:23-57, summed over the task's
// batches instead of keeping the last one): acc = beta * acc + alpha * f(src), f = x | x^2 | |x|, over a chunk table of
// (src, acc) pairs.  rows: src, acc; numel[t] = elements to touch (a prefix of acc when the class head has grown).
// Pure streaming, one owner thread per element.  beta == 0: acc is not read; alpha == 0: src is not read.
template <int OP>
__device__ __forceinline__ float cl_acc_value(float a, float x, float alpha, float beta, bool rd_src, bool rd_acc) {
  const float f = OP == 1 ? x * x : OP == 2 ? fabsf(x) : x;
  if (!rd_acc) return alpha * f;
  return rd_src ? __fmaf_rn(beta, a, alpha * f) : beta * a;
}

template <int OP>
__device__ __forceinline__ void cl_acc_scalar(const float* src, float* acc, long lo, long hi, float alpha, float beta,
                                              bool rd_src, bool rd_acc) {
  for (long i = lo + threadIdx.x; i < hi; i += OPT_THREADS) {
    const float x = rd_src ? src[i] : 0.f;
    const float a = rd_acc ? acc[i] : 0.f;
    acc[i] = cl_acc_value<OP>(a, x, alpha, beta, rd_src, rd_acc);
  }
}

template <int OP>
__global__ __launch_bounds__(OPT_THREADS) void cl_accumulate_kernel(MultiArgs a, float alpha, float beta) {
  const ChunkView c = chunk_view(a);
  const long cnt = c.cnt;
  const float* src = c.row<const float>(0);
  float* acc = c.row<float>(1);
  const bool rd_src = alpha != 0.f, rd_acc = beta != 0.f;
  // 16-byte accesses over the part where BOTH streams are 16-byte aligned: that needs the same misalignment on both (tensor
  // base pointers are arbitrary); then a scalar head of up to 3 elements, the wide body, a scalar tail.  Otherwise all scalar.
  const unsigned ma = (unsigned)(reinterpret_cast<uintptr_t>(acc) & 15), ms = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15);
  long head = cnt, nvec = 0;
  if (ma == ms && (ma & 3) == 0) {
    head = ((16 - ma) & 15) >> 2;
    if (head > cnt) head = cnt;
    nvec = (cnt - head) >> 2;
  }
  cl_acc_scalar<OP>(src, acc, 0, head, alpha, beta, rd_src, rd_acc);
  const float4* s4 = reinterpret_cast<const float4*>(src + head);
  float4* a4 = reinterpret_cast<float4*>(acc + head);
  for (long i = threadIdx.x; i < nvec; i += OPT_THREADS) {
    const float4 x = rd_src ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v = rd_acc ? a4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r;
    r.x = cl_acc_value<OP>(v.x, x.x, alpha, beta, rd_src, rd_acc);
    r.y = cl_acc_value<OP>(v.y, x.y, alpha, beta, rd_src, rd_acc);
    r.z = cl_acc_value<OP>(v.z, x.z, alpha, beta, rd_src, rd_acc);
    r.w = cl_acc_value<OP>(v.w, x.w, alpha, beta, rd_src, rd_acc);
    a4[i] = r;
  }
  cl_acc_scalar<OP>(src, acc, head + 4 * nvec, cnt, alpha, beta, rd_src, rd_acc);
}

// End of a task under Synaptic Intelligence: the path integral becomes importance, in place, ONE launch over all tensors.
//   Omega = Omega_old + max(omega, 0) / ((p - theta_start)^2 + xi) ; optpar = p ; omega = 0 ; theta_start = p
// rows: param, omega, theta_start, importance, optpar, each of numel[t] elements; importance held a value in its first
// numel_old[t] elements only (0: none yet; a prefix: the class head has grown), what lies behind them is not read.
// The quotient and the sum are formed in double and rounded once.  One owner thread per element, five streams, no atomics.
__global__ __launch_bounds__(OPT_THREADS) void si_consolidate_kernel(MultiArgs a, const long* __restrict__ numel_old, float xi) {
  const ChunkView c = chunk_view(a);
  const float* p = c.row<const float>(0);
  float* om = c.row<float>(1);
  float* ts = c.row<float>(2);
  float* f = c.row<float>(3);
  float* o = c.row<float>(4);
  const long old = numel_old[c.t] - c.off;       // elements of this chunk that carry an earlier importance
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) {
    const float pv = p[i];
    const double d = (double)pv - (double)ts[i];
    const double q = (double)fmaxf(om[i], 0.f) / (d * d + (double)xi);
    f[i] = (float)(i < old ? (double)f[i] + q : q);
    o[i] = pv;
    om[i] = 0.f;
    ts[i] = pv;
  }
}

// End of a task under RWalk.  rows: param, fisher F, score s, omega w, theta_ck; out_ptrs [2][n] = importance, optpar.
// Three launches, nothing read back by the host:
//   flush   the interval the last checkpoint left open is closed as the update kernel closes one:
//           s += max(w, 0) / (0.5 F d^2 + eps), d = p - theta_ck (double, rounded once) ; w = 0.
//           partial[c] = max F, partial[nchunks + c] = max s over chunk c (cnt == 0: two zeros).
//   finish  one block: out = {max F, max s} over the two runs of partials.
//   apply   importance = F / maxF + s / maxS (double, rounded once; a term whose max is 0 contributes 0) ; optpar = p ;
//           s = s / 2 ; theta_ck = p.  F is kept: its moving average runs on into the next task.
// The maxima propagate a NaN (fmaxf would drop it): a poisoned F or s poisons every importance instead of vanishing.
__device__ __forceinline__ float nan_max(float a, float b) { return (a > b || a != a) ? a : b; }

// every thread gets the nan_max of the block's x
__device__ __forceinline__ float block_nan_max(float x) {
  __shared__ float red[OPT_THREADS];
  red[threadIdx.x] = x;
  __syncthreads();
  for (int o = OPT_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] = nan_max(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();                               // red is reused by the next call
  return r;
}

__global__ __launch_bounds__(OPT_THREADS) void rwalk_flush_kernel(MultiArgs a, float eps, float* __restrict__ partial,
                                                                  int nchunks) {
  const ChunkView c = chunk_view(a);
  const float* p = c.row<const float>(0);
  const float* f = c.row<const float>(1);
  float* s = c.row<float>(2);
  float* w = c.row<float>(3);
  const float* ck = c.row<const float>(4);
  float mf = 0.f, ms = 0.f;
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) {
#pragma clang fp contract(off)
    const float fv = f[i];
    const double d = (double)p[i] - (double)ck[i];
    const double q = (double)fmaxf(w[i], 0.f) / (0.5 * (double)fv * d * d + (double)eps);
    const float sn = (float)((double)s[i] + q);
    s[i] = sn;
    w[i] = 0.f;
    mf = nan_max(mf, fv);
    ms = nan_max(ms, sn);
  }
  mf = block_nan_max(mf);
  ms = block_nan_max(ms);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = mf;
    partial[nchunks + blockIdx.x] = ms;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void rwalk_finish_kernel(const float* __restrict__ partial, int nchunks,
                                                                   float* __restrict__ out) {
  float mf = 0.f, ms = 0.f;
  for (int i = threadIdx.x; i < nchunks; i += OPT_THREADS) {
    mf = nan_max(mf, partial[i]);
    ms = nan_max(ms, partial[nchunks + i]);
  }
  mf = block_nan_max(mf);
  ms = block_nan_max(ms);
  if (threadIdx.x == 0) {
    out[0] = mf;
    out[1] = ms;
  }
}

__global__ __launch_bounds__(OPT_THREADS) void rwalk_apply_kernel(MultiArgs a, const long* __restrict__ out_ptrs,
                                                                  const float* __restrict__ out) {
  const ChunkView c = chunk_view(a);
  const float* p = c.row<const float>(0);
  const float* f = c.row<const float>(1);
  float* s = c.row<float>(2);
  float* ck = c.row<float>(4);
  float* imp = reinterpret_cast<float*>(out_ptrs[c.t]) + c.off;
  float* opt = reinterpret_cast<float*>(out_ptrs[c.n + c.t]) + c.off;
  const float mf = out[0], ms = out[1];
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) {
#pragma clang fp contract(off)
    const float pv = p[i], sv = s[i];
    const double tf = mf == 0.f ? 0.0 : (double)f[i] / (double)mf;      // (a NaN max is not 0: it reaches the quotient)
    const double tsc = ms == 0.f ? 0.0 : (double)sv / (double)ms;
    imp[i] = (float)(tf + tsc);
    opt[i] = pv;
    s[i] = 0.5f * sv;
    ck[i] = pv;
  }
}

// A-GEM (Chaudhry et al., ICLR 2019, "Efficient Lifelong Learning with A-GEM"): the step's gradient g is projected against the
// replay memory's gradient r when the two conflict:  g <- g - (g.r / r.r) r  if g.r < 0.  rows: grad (projected in place), ref.
// Three launches, the branch is taken on the device:
//   dot     partial[c] = sum over chunk c of g r, partial[nchunks + c] = of r r: ONE read of the two streams, fp32 per-thread sums
//           in sqnorm_kernel's order, then its wave / block tree (block_sum_to, once per sum with a barrier between: it owns one
//           shared array).  A chunk with cnt == 0 writes two zeros.
//   finish  one block: both runs summed in double; out = {g.r, r.r, alpha}, alpha = (float)(g.r / r.r) if g.r < 0 && r.r > 0,
//           else 0 (a NaN dot fails the comparison: the gradient is left as it is)
//   apply   alpha == 0: every block returns without a load or a store.  Otherwise g[i] = fmaf(-alpha, r[i], g[i]), one owner
//           thread per element, in cl_accumulate_kernel's access pattern (16-byte where grad and ref share a misalignment).
__global__ __launch_bounds__(OPT_THREADS) void agem_dot_kernel(MultiArgs a, float* __restrict__ partial, int nchunks) {
  const ChunkView c = chunk_view(a);
  const float* g = c.row<const float>(0);
  const float* r = c.row<const float>(1);
  float sd = 0.f, sr = 0.f;
  for (long i = threadIdx.x; i < c.cnt; i += OPT_THREADS) {
    const float rv = r[i];
    sd += g[i] * rv;
    sr += rv * rv;
  }
  block_sum_to(sd, partial + blockIdx.x);
  __syncthreads();                               // thread 0 has read the shared array of the first sum
  block_sum_to(sr, partial + nchunks + blockIdx.x);
}

__global__ __launch_bounds__(OPT_THREADS) void agem_finish_kernel(const float* __restrict__ partial, int nchunks,
                                                                  float* __restrict__ out) {
  const double dot = partials_sum(partial, nchunks);
  __syncthreads();                               // every thread has read red[0] of the first sum
  const double rr = partials_sum(partial + nchunks, nchunks);
  if (threadIdx.x == 0) {
    out[0] = (float)dot;
    out[1] = (float)rr;
    out[2] = (dot < 0.0 && rr > 0.0) ? (float)(dot / rr) : 0.f;
  }
}

__device__ __forceinline__ void agem_apply_scalar(const float* r, float* g, long lo, long hi, float nalpha) {
  for (long i = lo + threadIdx.x; i < hi; i += OPT_THREADS) g[i] = __fmaf_rn(nalpha, r[i], g[i]);
}

__global__ __launch_bounds__(OPT_THREADS) void agem_apply_kernel(MultiArgs a, const float* __restrict__ out) {
  const float alpha = out[2];
  if (alpha == 0.f) return;                      // no conflict: grad keeps its bits, no traffic
  const float nalpha = -alpha;
  const ChunkView c = chunk_view(a);
  const long cnt = c.cnt;
  float* g = c.row<float>(0);
  const float* r = c.row<const float>(1);
  // as cl_accumulate_kernel: 16-byte accesses over the part where BOTH streams are 16-byte aligned, scalar head and tail
  const unsigned mg = (unsigned)(reinterpret_cast<uintptr_t>(g) & 15), mr = (unsigned)(reinterpret_cast<uintptr_t>(r) & 15);
  long head = cnt, nvec = 0;
  if (mg == mr && (mg & 3) == 0) {
    head = ((16 - mg) & 15) >> 2;
    if (head > cnt) head = cnt;
    nvec = (cnt - head) >> 2;
  }
  agem_apply_scalar(r, g, 0, head, nalpha);
  const float4* r4 = reinterpret_cast<const float4*>(r + head);
  float4* g4 = reinterpret_cast<float4*>(g + head);
  for (long i = threadIdx.x; i < nvec; i += OPT_THREADS) {
    const float4 x = r4[i];
    float4 v = g4[i];
    v.x = __fmaf_rn(nalpha, x.x, v.x);
    v.y = __fmaf_rn(nalpha, x.y, v.y);
    v.z = __fmaf_rn(nalpha, x.z, v.z);
    v.w = __fmaf_rn(nalpha, x.w, v.w);
    g4[i] = v;
  }
  agem_apply_scalar(r, g, head + 4 * nvec, cnt, nalpha);
}

struct F16Vals { float v[16]; };
__global__ void store_f32_kernel(float* __restrict__ dst, F16Vals vals, int n) {
  if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

// the MultiArgs of a table whose entry point reads `rows` rows; false: VILCO_ERR_BADARG
bool table_args(const vilco_chunk_table* t, int rows, const int32_t* group, MultiArgs* a) {
  if (!t || !t->ptrs || !t->numel || !t->chunk_tensor || !t->chunk_off) return false;
  if (t->n < 0 || t->nchunks < 0 || t->chunk <= 0 || t->rows < rows) return false;
  *a = MultiArgs{reinterpret_cast<const long*>(t->ptrs), reinterpret_cast<const long*>(t->numel), t->chunk_tensor,
                 reinterpret_cast<const long*>(t->chunk_off), group, t->n, t->chunk};
  return true;
}

}  // namespace

// dst[0..n) = vals[0..n) (n <= 16 host floats, carried as kernel arguments: no staging buffer whose lifetime the caller
// would have to manage, stream-ordered with the replays that read dst).  The learning rates of a captured step.
extern "C" int vilco_store_f32(float* dst, const float* vals, int32_t n, void* stream) {
  if (!dst || !vals || n < 0 || n > 16) return VILCO_ERR_BADARG;
  if (n == 0) return VILCO_OK;
  F16Vals v;
  for (int i = 0; i < 16; ++i) v.v[i] = i < n ? vals[i] : 0.f;
  hipLaunchKernelGGL(store_f32_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), dst, v, n);
  return vilco_launch_status();
}

extern "C" int vilco_cl_penalty(const vilco_chunk_table* table, float lambda, int32_t shared_params, float* partial, float* out,
                                void* stream) {
  MultiArgs a;
  if (!table_args(table, 4, nullptr, &a) || !partial || !out) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(table->nchunks), block(OPT_THREADS);
  if (table->nchunks > 0) {
    if (shared_params) hipLaunchKernelGGL(cl_penalty_kernel<true>, grid, block, 0, s, a, lambda, partial);
    else hipLaunchKernelGGL(cl_penalty_kernel<false>, grid, block, 0, s, a, lambda, partial);
  }
  hipLaunchKernelGGL(scaled_sum_kernel, dim3(1), block, 0, s, partial, table->nchunks, lambda, out);
  return vilco_launch_status();
}

extern "C" int vilco_cl_accumulate(const vilco_chunk_table* table, int32_t op, float alpha, float beta, void* stream) {
  MultiArgs a;
  if (!table_args(table, 2, nullptr, &a) || op < 0 || op > 2) return VILCO_ERR_BADARG;
  if (table->nchunks == 0) return VILCO_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(table->nchunks), block(OPT_THREADS);
  if (op == 0) hipLaunchKernelGGL(cl_accumulate_kernel<0>, grid, block, 0, s, a, alpha, beta);
  else if (op == 1) hipLaunchKernelGGL(cl_accumulate_kernel<1>, grid, block, 0, s, a, alpha, beta);
  else hipLaunchKernelGGL(cl_accumulate_kernel<2>, grid, block, 0, s, a, alpha, beta);
  return vilco_launch_status();
}

extern "C" int vilco_grad_norm(const vilco_chunk_table* table, float max_norm, float* partial, float* norm_coef, void* stream) {
  MultiArgs a;
  if (!table_args(table, 2, nullptr, &a) || !partial || !norm_coef) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nchunks = table->nchunks;
  if (nchunks > 0) hipLaunchKernelGGL(sqnorm_kernel, dim3(nchunks), dim3(OPT_THREADS), 0, s, a, partial);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(OPT_THREADS), 0, s, partial, nchunks, max_norm, norm_coef);
  return vilco_launch_status();
}

extern "C" int vilco_agem_project(const vilco_chunk_table* table, float* partial, float* out, void* stream) {
  MultiArgs a;
  if (!table_args(table, 2, nullptr, &a) || !partial || !out) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nchunks = table->nchunks;
  const dim3 grid(nchunks), block(OPT_THREADS);
  if (nchunks > 0) hipLaunchKernelGGL(agem_dot_kernel, grid, block, 0, s, a, partial, nchunks);
  hipLaunchKernelGGL(agem_finish_kernel, dim3(1), block, 0, s, partial, nchunks, out);
  if (nchunks > 0) hipLaunchKernelGGL(agem_apply_kernel, grid, block, 0, s, a, out);
  return vilco_launch_status();
}

// the update launch of vilco_optim_step (rw null) and vilco_optim_step_rwalk
static int optim_launch(const vilco_optim_desc* d, const RwalkArgs* rw, void* stream) {
  const int32_t kind = d->kind, ngroups = d->ngroups;
  MultiArgs a;
  if (!table_args(&d->table, kind == 1 ? 3 : 4, d->group, &a) || !d->group || !d->lr || !d->wd) return VILCO_ERR_BADARG;
  if (ngroups < 1 || ngroups > 8 || !d->tensor_step || (kind != 0 && kind != 1)) return VILCO_ERR_BADARG;
  if (d->table.nchunks == 0) return VILCO_OK;
  Hyper h;
  for (int i = 0; i < 8; ++i) { h.lr[i] = i < ngroups ? d->lr[i] : 0.f; h.wd[i] = i < ngroups ? d->wd[i] : 0.f; }
  h.beta1 = d->beta1; h.beta2 = d->beta2; h.eps = d->eps;
  h.log_beta1 = (float)log((double)d->beta1); h.log_beta2 = (float)log((double)d->beta2);
  h.momentum = d->momentum;
  h.tstep = d->tensor_step;
  h.lr_dev = d->lr_dev;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long* si = reinterpret_cast<const long*>(d->si_ptrs);
  const dim3 grid(d->table.nchunks), block(OPT_THREADS);
  if (rw && kind == 0) hipLaunchKernelGGL(adamw_rwalk_kernel, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si, *rw);
  else if (rw) hipLaunchKernelGGL(sgd_rwalk_kernel, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si, *rw);
  else if (kind == 0 && si) hipLaunchKernelGGL(adamw_kernel<true>, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si);
  else if (kind == 0) hipLaunchKernelGGL(adamw_kernel<false>, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si);
  else if (si) hipLaunchKernelGGL(sgd_kernel<true>, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si);
  else hipLaunchKernelGGL(sgd_kernel<false>, grid, block, 0, s, a, h, d->norm_coef, d->chunk_amax, si);
  return vilco_launch_status();
}

extern "C" int vilco_optim_step(const vilco_optim_desc* d, void* stream) {
  if (!d) return VILCO_ERR_BADARG;
  return optim_launch(d, nullptr, stream);
}

extern "C" int vilco_optim_step_rwalk(const vilco_rwalk_step_desc* d, void* stream) {
  if (!d) return VILCO_ERR_BADARG;
  if (!d->optim.si_ptrs || !d->rw_ptrs || !d->tick) return VILCO_ERR_BADARG;
  if (!(d->alpha > 0.f && d->alpha <= 1.f) || !(d->eps > 0.f) || d->delta_t < 1) return VILCO_ERR_BADARG;
  const RwalkArgs rw{reinterpret_cast<const long*>(d->rw_ptrs), d->tick, d->alpha, d->eps, d->delta_t};
  return optim_launch(&d->optim, &rw, stream);
}

extern "C" int vilco_rwalk_consolidate(const vilco_rwalk_desc* d, void* stream) {
  if (!d) return VILCO_ERR_BADARG;
  MultiArgs a;
  if (!table_args(&d->table, 5, nullptr, &a) || d->table.n <= 0 || !d->out_ptrs || !d->partial || !d->out) return VILCO_ERR_BADARG;
  if (!(d->eps > 0.f)) return VILCO_ERR_BADARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nchunks = d->table.nchunks;
  if (nchunks == 0) return VILCO_OK;             // no element: no state to flush, no importance to write
  const dim3 grid(nchunks), block(OPT_THREADS);
  hipLaunchKernelGGL(rwalk_flush_kernel, grid, block, 0, s, a, d->eps, d->partial, nchunks);
  hipLaunchKernelGGL(rwalk_finish_kernel, dim3(1), block, 0, s, d->partial, nchunks, d->out);
  hipLaunchKernelGGL(rwalk_apply_kernel, grid, block, 0, s, a, reinterpret_cast<const long*>(d->out_ptrs), d->out);
  return vilco_launch_status();
}

extern "C" int vilco_si_consolidate(const vilco_si_desc* d, void* stream) {
  if (!d) return VILCO_ERR_BADARG;
  MultiArgs a;
  if (!table_args(&d->table, 5, nullptr, &a) || !d->numel_old || d->table.n <= 0 || !(d->xi > 0.f)) return VILCO_ERR_BADARG;
  if (d->table.nchunks == 0) return VILCO_OK;
  hipLaunchKernelGGL(si_consolidate_kernel, dim3(d->table.nchunks), dim3(OPT_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a,
                     reinterpret_cast<const long*>(d->numel_old), d->xi);
  return vilco_launch_status();
}
