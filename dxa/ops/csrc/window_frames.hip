// Moment states of SQL window frames for gfx950: for every row i (rows in window order) the state of the counted
// rows of its frame x[a[i] .. b[i]] — the variance family's (n, mean, M2), skewness / kurtosis' (n, mean, M2, M3,
// M4) or the covariance family's (n, mean_x, mean_y, Cxy, M2x, M2y) — written as f64 [words][n].  The window
// evaluator (engine/windowfn.py) turns a state into stddev / variance / skewness / kurtosis / covar / corr.
//
// Two entry points, both one thread per row with a grid-stride loop:
//   * dxa_frame_moments_direct — short frames, ONE launch: pass 1 over the frame gives the count and the mean(s),
//     pass 2 the central sums about that mean.  Exact two-pass arithmetic, no merge; neighbouring rows' frames
//     overlap, so the second read is served from cache.
//   * dxa_frame_moments_levels — any frame length, one launch per level k = 0 .. bit_length(maxlen) - 1.  Level k is
//     the state of the run of 2^k rows starting at every row (clipped at n).  A frame is cut into power-of-two runs
//     by the bits of its length, lowest bit first, walking forward from a[i]: launch k merges level_k[pos] into the
//     row's state when bit k of the length is set, and builds level_{k+1}[i] = merge(level_k[i], level_k[i + 2^k])
//     into the other of two ping-pong buffers.  Every run a frame uses lies inside the frame, so partition
//     boundaries need no special case (level blocks that straddle one are built and never read).
//
// States merge pairwise (Chan et al.); nothing is computed as sum(x^2) - sum(x)^2 / n.  Level 0 of a counted row is
// (1, x, x - x, ..): the x - x makes a frame holding NaN or +-inf NaN, as the two-pass form gives.  A row that is not
// counted (NULL argument) is the identity, all words 0.
//
// Every index is checked before its load: a and b are clamped to [0, n), an empty frame (a > b) loads nothing,
// i + 2^k >= n merges the identity.  No atomics, no LDS, no inter-workgroup traffic: a thread writes its own row's
// words only.
#include "dxa_common.h"

namespace {

enum : int { kVar = 0, kMom = 1, kCo = 2 };

template <int KIND>
struct State {
  static constexpr int kWords = KIND == kVar ? 3 : KIND == kMom ? 5 : 6;
  double w[kWords];
};

template <int KIND>
__device__ __forceinline__ State<KIND> identity() {
  State<KIND> s;
#pragma unroll
  for (int j = 0; j < State<KIND>::kWords; ++j) s.w[j] = 0.0;
  return s;
}

template <int KIND>
__device__ __forceinline__ State<KIND> load_state(const double* p, int64_t n, int64_t i) {
  State<KIND> s;
#pragma unroll
  for (int j = 0; j < State<KIND>::kWords; ++j) s.w[j] = p[(int64_t)j * n + i];
  return s;
}

template <int KIND>
__device__ __forceinline__ void store_state(double* p, int64_t n, int64_t i, const State<KIND>& s) {
#pragma unroll
  for (int j = 0; j < State<KIND>::kWords; ++j) p[(int64_t)j * n + i] = s.w[j];
}

// Level 0: the state of row i alone (0 <= i < n).
template <int KIND>
__device__ __forceinline__ State<KIND> row_state(const double* x, const double* y, const uint8_t* valid, int64_t i) {
  State<KIND> s = identity<KIND>();
  if (valid != nullptr && valid[i] == 0) return s;
  const double xv = x[i];
  const double zx = xv - xv;                 // 0, or NaN for a non-finite value
  s.w[0] = 1.0;
  s.w[1] = xv;
  if (KIND == kCo) {
    const double yv = y[i];
    const double zy = yv - yv;
    s.w[2] = yv;
    s.w[3] = zx * zy;
    s.w[4] = zx;
    s.w[5] = zy;
  } else {
#pragma unroll
    for (int j = 2; j < State<KIND>::kWords; ++j) s.w[j] = zx;
  }
  return s;
}

// A is the left run, B the right one.
template <int KIND>
__device__ __forceinline__ State<KIND> merge(const State<KIND>& A, const State<KIND>& B) {
  const double na = A.w[0], nb = B.w[0];
  if (nb == 0.0) return A;
  if (na == 0.0) return B;
  const double n = na + nb;
  State<KIND> r;
  r.w[0] = n;
  if (KIND == kCo) {
    const double dx = B.w[1] - A.w[1], dy = B.w[2] - A.w[2];
    const double f = na * nb / n;
    r.w[1] = A.w[1] + dx * nb / n;
    r.w[2] = A.w[2] + dy * nb / n;
    r.w[3] = A.w[3] + B.w[3] + dx * dy * f;
    r.w[4] = A.w[4] + B.w[4] + dx * dx * f;
    r.w[5] = A.w[5] + B.w[5] + dy * dy * f;
  } else {
    const double d = B.w[1] - A.w[1];
    const double d2 = d * d;
    r.w[1] = A.w[1] + d * nb / n;
    r.w[2] = A.w[2] + B.w[2] + d2 * na * nb / n;
    if (KIND == kMom) {
      const double n2 = n * n;
      r.w[3] = A.w[3] + B.w[3] + d2 * d * na * nb * (na - nb) / n2 + 3.0 * d * (na * B.w[2] - nb * A.w[2]) / n;
      r.w[4] = A.w[4] + B.w[4] + d2 * d2 * na * nb * (na * na - na * nb + nb * nb) / (n2 * n) +
               6.0 * d2 * (na * na * B.w[2] + nb * nb * A.w[2]) / n2 + 4.0 * d * (na * B.w[3] - nb * A.w[3]) / n;
    }
  }
  return r;
}

// The frame of row i clipped to [0, n): first row and length (0: empty).
__device__ __forceinline__ void frame_of(const int64_t* a, const int64_t* b, int64_t n, int64_t i, int64_t& lo,
                                         int64_t& len) {
  int64_t l = a[i], h = b[i];
  lo = 0;
  len = 0;
  if (l > h) return;
  if (l < 0) l = 0;
  if (h > n - 1) h = n - 1;
  if (l > h) return;
  lo = l;
  len = h - l + 1;
}

template <int KIND>
__global__ __launch_bounds__(256) void frame_direct_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                           const uint8_t* __restrict__ valid,
                                                           const int64_t* __restrict__ a,
                                                           const int64_t* __restrict__ b, int64_t n,
                                                           double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, len;
    frame_of(a, b, n, i, lo, len);
    const int64_t end = lo + len;                       // <= n
    double cnt = 0.0, sx = 0.0, sy = 0.0;
    for (int64_t j = lo; j < end; ++j) {
      if (valid != nullptr && valid[j] == 0) continue;
      cnt += 1.0;
      sx += x[j];
      if (KIND == kCo) sy += y[j];
    }
    State<KIND> s = identity<KIND>();
    if (cnt > 0.0) {
      const double mx = sx / cnt, my = sy / cnt;
      double m2 = 0.0, m3 = 0.0, m4 = 0.0, cxy = 0.0, m2y = 0.0;
      for (int64_t j = lo; j < end; ++j) {
        if (valid != nullptr && valid[j] == 0) continue;
        const double dx = x[j] - mx;
        const double d2 = dx * dx;
        m2 += d2;
        if (KIND == kMom) {
          m3 += d2 * dx;
          m4 += d2 * d2;
        }
        if (KIND == kCo) {
          const double dy = y[j] - my;
          cxy += dx * dy;
          m2y += dy * dy;
        }
      }
      s.w[0] = cnt;
      s.w[1] = mx;
      if (KIND == kCo) {
        s.w[2] = my;
        s.w[3] = cxy;
        s.w[4] = m2;
        s.w[5] = m2y;
      } else {
        s.w[2] = m2;
        if (KIND == kMom) {
          s.w[3] = m3;
          s.w[4] = m4;
        }
      }
    }
    store_state<KIND>(out, n, i, s);
  }
}

// One level.  FIRST (k = 0): level 0 is read from the rows themselves and every row's state is initialised; later
// levels read `src` (level k) and touch the state only where bit k of the frame length is set.  `dst` (level k + 1)
// is null at the last level.
template <int KIND, bool FIRST>
__global__ __launch_bounds__(256) void frame_level_kernel(const double* __restrict__ x, const double* __restrict__ y,
                                                          const uint8_t* __restrict__ valid,
                                                          const int64_t* __restrict__ a,
                                                          const int64_t* __restrict__ b, int64_t n, int k,
                                                          const double* __restrict__ src, double* __restrict__ dst,
                                                          double* __restrict__ out) {
  const int64_t step = (int64_t)1 << k;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo, len;
    frame_of(a, b, n, i, lo, len);
    if (FIRST) {
      // bit 0 set: len >= 1, so lo is a row of the frame
      store_state<KIND>(out, n, i, (len & 1) ? row_state<KIND>(x, y, valid, lo) : identity<KIND>());
    } else if ((len >> k) & 1) {
      // the runs of the lower bits end at pos; pos + step <= lo + len <= n
      const int64_t pos = lo + (len & (step - 1));
      store_state<KIND>(out, n, i, merge<KIND>(load_state<KIND>(out, n, i), load_state<KIND>(src, n, pos)));
    }
    if (dst != nullptr) {
      const int64_t j = i + step;
      State<KIND> A, B;
      if (FIRST) {
        A = row_state<KIND>(x, y, valid, i);
        B = j < n ? row_state<KIND>(x, y, valid, j) : identity<KIND>();
      } else {
        A = load_state<KIND>(src, n, i);
        B = j < n ? load_state<KIND>(src, n, j) : identity<KIND>();
      }
      store_state<KIND>(dst, n, i, merge<KIND>(A, B));
    }
  }
}

inline int words_of(int kind) { return kind == kVar ? 3 : kind == kMom ? 5 : kind == kCo ? 6 : 0; }

template <int KIND>
int launch_direct(const double* x, const double* y, const uint8_t* valid, const int64_t* a, const int64_t* b,
                  int64_t n, double* out, hipStream_t st) {
  hipLaunchKernelGGL(frame_direct_kernel<KIND>, dim3(dxa_blocks(n, 256)), dim3(256), 0, st, x, y, valid, a, b, n,
                     out);
  return (int)hipGetLastError();
}

template <int KIND>
int launch_levels(const double* x, const double* y, const uint8_t* valid, const int64_t* a, const int64_t* b,
                  int64_t n, int levels, double* scratch, double* out, hipStream_t st) {
  const int64_t plane = (int64_t)State<KIND>::kWords * n;
  const dim3 grid(dxa_blocks(n, 256)), block(256);
  for (int k = 0; k < levels; ++k) {
    double* dst = k + 1 < levels ? scratch + (int64_t)(k & 1) * plane : nullptr;
    if (k == 0) {
      hipLaunchKernelGGL((frame_level_kernel<KIND, true>), grid, block, 0, st, x, y, valid, a, b, n, k,
                         (const double*)nullptr, dst, out);
    } else {
      const double* src = scratch + (int64_t)((k - 1) & 1) * plane;
      hipLaunchKernelGGL((frame_level_kernel<KIND, false>), grid, block, 0, st, x, y, valid, a, b, n, k, src, dst,
                         out);
    }
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return 0;
}

}  // namespace

// kind: 0 variance (3 words), 1 moments (5), 2 co-moments (6).  x, a, b: n entries; y: n entries for kind 2, else
// unused; valid: n bytes or null (every row counted); out: words * n doubles.
DXA_API int dxa_frame_moments_direct(const double* x, const double* y, const uint8_t* valid, const int64_t* a,
                                     const int64_t* b, int64_t n, int32_t kind, double* out, void* st) {
  if (n < 0 || words_of(kind) == 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (x == nullptr || a == nullptr || b == nullptr || out == nullptr || (kind == kCo && y == nullptr))
    return (int)hipErrorInvalidValue;
  switch (kind) {
    case kVar: return launch_direct<kVar>(x, y, valid, a, b, n, out, (hipStream_t)st);
    case kMom: return launch_direct<kMom>(x, y, valid, a, b, n, out, (hipStream_t)st);
    default: return launch_direct<kCo>(x, y, valid, a, b, n, out, (hipStream_t)st);
  }
}

// maxlen: the longest frame length (>= 1; frames longer than it lose their high runs).  scratch: 2 * words * n
// doubles, needed when maxlen > 1.
DXA_API int dxa_frame_moments_levels(const double* x, const double* y, const uint8_t* valid, const int64_t* a,
                                     const int64_t* b, int64_t n, int32_t kind, int64_t maxlen, double* scratch,
                                     double* out, void* st) {
  if (n < 0 || words_of(kind) == 0 || maxlen <= 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (x == nullptr || a == nullptr || b == nullptr || out == nullptr || (kind == kCo && y == nullptr))
    return (int)hipErrorInvalidValue;
  if (maxlen > n) maxlen = n;                          // frames are clipped to [0, n)
  int levels = 0;
  while (levels < 63 && ((int64_t)1 << levels) <= maxlen) ++levels;
  if (levels > 1 && scratch == nullptr) return (int)hipErrorInvalidValue;
  switch (kind) {
    case kVar: return launch_levels<kVar>(x, y, valid, a, b, n, levels, scratch, out, (hipStream_t)st);
    case kMom: return launch_levels<kMom>(x, y, valid, a, b, n, levels, scratch, out, (hipStream_t)st);
    default: return launch_levels<kCo>(x, y, valid, a, b, n, levels, scratch, out, (hipStream_t)st);
  }
}
