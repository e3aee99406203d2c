// The evaluation report on the device (timewarp_amd/evaluate.py): pair distances, per-column ranges and per-column histograms of a
// strided float32 matrix or of the distances of atom pairs computed on the fly.  The entry points are declared in
// include/timewarp_hip.h, which also states what each computes; this file holds the kernels and the argument checks.
#include "tw_common.h"

namespace tw {
namespace {

// ---- the one distance ------------------------------------------------------------------------------------------------------------
// fp64 from the float32 coordinates in the order the header states; every caller (tw_pair_distances, the fused range and histogram)
// goes through this function, so the fused kernels bin the very float32 the materialising call stores.
__device__ __forceinline__ float pair_distance_f32(const float* __restrict__ row, int i, int j) {
  const float* a = row + 3 * (int64_t)i;
  const float* b = row + 3 * (int64_t)j;
  const double t0 = (double)a[0] - (double)b[0], t1 = (double)a[1] - (double)b[1], t2 = (double)a[2] - (double)b[2];
  double d2 = __dmul_rn(t0, t0);
  d2 = fma(t1, t1, d2);
  d2 = fma(t2, t2, d2);
  return (float)sqrt(d2);
}

constexpr int kDistThreads = 256;
constexpr int kDistItems = 2048;  // (row, pair) items of one workgroup, more when one row has more pairs

__global__ __launch_bounds__(kDistThreads) void pair_distances_kernel(const float* __restrict__ coords, const int* __restrict__ pairs,
                                                                      int n_pairs, float* __restrict__ out, int64_t n_rows, int n_atoms,
                                                                      int rows_per_block) {
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int rows = (int)(n_rows - row0 < rows_per_block ? n_rows - row0 : rows_per_block);
  const int items = rows * n_pairs;
  for (int it = threadIdx.x; it < items; it += kDistThreads) {
    const int r = it / n_pairs, p = it - r * n_pairs;
    out[row0 * n_pairs + it] = pair_distance_f32(coords + (row0 + r) * n_atoms * 3, pairs[2 * p], pairs[2 * p + 1]);
  }
}

// ---- column sources ----------------------------------------------------------------------------------------------------------------
// What the range and histogram kernels read: column c of row r.  A thread keeps ONE column for its whole life (bind), so whatever
// the column needs - a base pointer, a pair of atom indices - lives in registers; kUnroll values are loaded before any is consumed.
struct StridedSource {
  static constexpr int kUnroll = 8;
  const float* X;
  int64_t ld, col_stride;
  struct Column {
    const float* p;
    int64_t ld;
    __device__ __forceinline__ float load(int64_t r) const { return p[r * ld]; }
  };
  __device__ __forceinline__ Column bind(int64_t c) const { return Column{X + c * col_stride, ld}; }
};

struct PairSource {
  static constexpr int kUnroll = 2;
  const float* coords;
  const int* pairs;
  int n_atoms;
  struct Column {
    const float* coords;
    int64_t row_floats;
    int i, j;
    __device__ __forceinline__ float load(int64_t r) const { return pair_distance_f32(coords + r * row_floats, i, j); }
  };
  __device__ __forceinline__ Column bind(int64_t c) const { return Column{coords, (int64_t)n_atoms * 3, pairs[2 * c], pairs[2 * c + 1]}; }
};

// ---- geometry shared by the two kernels -------------------------------------------------------------------------------------------
// A workgroup owns one tile of W <= kColThreads consecutive columns and every gridDim.y-th block of P = kColThreads / W rows: thread
// t is column t % W of the tile and row phase t / W (threads with phase >= P idle: fewer than W of kColThreads), so consecutive
// threads read consecutive columns of one row and, for a one-column tile, consecutive rows.  The persistent loop advances by
// gridDim.y P rows; its trip count is the workgroup's, the same for every thread (the histogram's wave votes need that).
constexpr int kColThreads = 512;
constexpr int kColTargetWgs = 1024;      // workgroups of a launch: four per CU, fewer than that only when there are fewer row blocks
constexpr int kHistLdsBytes = 64 * 1024;  // the dynamic LDS a launch gets without opting in
constexpr int kRangeTile = 256;
constexpr int64_t kMaxTiles = 1ll << 20;
constexpr int64_t kMaxRows = (1ll << 32) - 1;  // a workgroup's u32 counters cannot wrap

// columns of a histogram tile: n_bins counters and the three outside counters per column, u32, in kHistLdsBytes
__host__ __device__ inline int hist_tile(int n_bins) {
  const int fit = kHistLdsBytes / ((n_bins + 3) * 4);
  return fit > kColThreads ? kColThreads : fit;
}

int rows_grid(int64_t n_rows, int W, int64_t n_tiles) {
  const int P = kColThreads / W;
  const int64_t row_blocks = (n_rows + P - 1) / P;
  int64_t want = (kColTargetWgs + n_tiles - 1) / n_tiles;
  if (want > row_blocks) want = row_blocks;
  return (int)(want < 1 ? 1 : want);
}

// ---- ranges ------------------------------------------------------------------------------------------------------------------------
// float32 -> u32 whose unsigned order is the float order (-inf lowest, -0 below +0, +inf highest), so min and max are INTEGER atomics:
// exact, order-independent, and the same bits whatever the split of the rows.  out_lo / out_hi hold keys between the three launches
// of a call (range_init_kernel, range_kernel, range_decode_kernel, in stream order) and floats after the last.
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ __launch_bounds__(256) void range_init_kernel(unsigned* __restrict__ lo, unsigned* __restrict__ hi,
                                                         unsigned long long* __restrict__ nonfinite, int n_cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < n_cols) lo[c] = order_key(INFINITY), hi[c] = order_key(-INFINITY), nonfinite[c] = 0ull;
}

__global__ __launch_bounds__(256) void range_decode_kernel(unsigned* __restrict__ lo, unsigned* __restrict__ hi, int n_cols) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < n_cols) {
    const float l = order_value(lo[c]), h = order_value(hi[c]);
    ((float*)lo)[c] = l, ((float*)hi)[c] = h;
  }
}

template <typename Src>
__global__ __launch_bounds__(kColThreads) void range_kernel(Src src, int64_t n_rows, int n_cols, unsigned* __restrict__ out_lo,
                                                            unsigned* __restrict__ out_hi, unsigned long long* __restrict__ out_nonfinite) {
  __shared__ unsigned s_lo[kRangeTile], s_hi[kRangeTile], s_nf[kRangeTile];
  const int c0 = blockIdx.x * kRangeTile;
  const int W = n_cols - c0 < kRangeTile ? n_cols - c0 : kRangeTile;
  const int P = kColThreads / W;
  const int tid = threadIdx.x, tx = tid % W, ty = tid / W;
  if (tid < W) s_lo[tid] = order_key(INFINITY), s_hi[tid] = order_key(-INFINITY), s_nf[tid] = 0u;
  __syncthreads();
  if (ty < P) {
    const typename Src::Column col = src.bind(c0 + tx);
    const int64_t step = (int64_t)gridDim.y * P;
    unsigned lo = order_key(INFINITY), hi = order_key(-INFINITY), nf = 0u;
    for (int64_t r = (int64_t)blockIdx.y * P + ty; r < n_rows; r += step * Src::kUnroll) {
      float x[Src::kUnroll];
#pragma unroll
      for (int u = 0; u < Src::kUnroll; ++u) x[u] = r + u * step < n_rows ? col.load(r + u * step) : 0.f;
#pragma unroll
      for (int u = 0; u < Src::kUnroll; ++u) {
        if (r + u * step >= n_rows) continue;
        if (fabsf(x[u]) < INFINITY) {  // finite: false for NaN and for +-inf
          const unsigned k = order_key(x[u]);
          lo = k < lo ? k : lo, hi = k > hi ? k : hi;
        } else {
          ++nf;
        }
      }
    }
    atomicMin(&s_lo[tx], lo);
    atomicMax(&s_hi[tx], hi);
    if (nf) atomicAdd(&s_nf[tx], nf);
  }
  __syncthreads();
  if (tid < W) {
    atomicMin(&out_lo[c0 + tid], s_lo[tid]);
    atomicMax(&out_hi[c0 + tid], s_hi[tid]);
    if (s_nf[tid]) atomicAdd(&out_nonfinite[c0 + tid], (unsigned long long)s_nf[tid]);
  }
}

// ---- histograms --------------------------------------------------------------------------------------------------------------------
// The bin of x in the table e[0 .. n_bins] (strictly increasing, e[0] <= x <= e[n_bins]): a uniform estimate from the two outer edges,
// clamped, then a walk against the table until e[i] <= x < e[i + 1] - or i = n_bins - 1, where x == e[n_bins] stays (the closed last
// bin).  The result is the table's alone: the estimate only decides how far the walk is (at most one step for np.linspace edges).
__device__ __forceinline__ int find_bin(double x, const double* __restrict__ e, int n_bins, double e0, double scale) {
  double t = (x - e0) * scale;
  t = fmin(fmax(t, 0.0), (double)(n_bins - 1));  // fmax(NaN, 0) = 0: a degenerate scale only lengthens the walk
  int i = (int)t;
  while (i > 0 && x < e[i]) --i;
  while (i < n_bins - 1 && x >= e[i + 1]) ++i;
  return i;
}

// LDS: counters [n_bins + 3][W] u32, bin-major (the lanes of a wave are different columns at nearby bins: consecutive banks), rows
// n_bins .. n_bins + 2 the below / above / NaN counters.  AGG (tiles narrower than a wave, where several lanes of a wave share a
// column and a bond length or an energy sends them all to a handful of counters): up to kAggRounds times the wave elects the first
// pending lane, every lane with the same counter retires, and the elected lane adds their number in one LDS atomic; what is still
// pending after that (a spread-out column) goes to plain LDS atomics.  The merge adds every non-zero counter to the caller's int64
// array with one 64-bit integer atomic: integer sums do not depend on order, so a call is bit-reproducible.
constexpr int kAggRounds = 4;

template <typename Src, bool AGG>
__global__ __launch_bounds__(kColThreads) void histogram_kernel(Src src, int64_t n_rows, int n_cols, const double* __restrict__ edges,
                                                                int n_bins, int tile, unsigned long long* __restrict__ counts,
                                                                unsigned long long* __restrict__ outside) {
  extern __shared__ unsigned hist[];
  const int c0 = blockIdx.x * tile;
  const int W = n_cols - c0 < tile ? n_cols - c0 : tile;
  const int P = kColThreads / W;
  const int tid = threadIdx.x, tx = tid % W, ty = tid / W;
  const int slots = (n_bins + 3) * W;
  for (int s = tid; s < slots; s += kColThreads) hist[s] = 0u;
  __syncthreads();

  const bool live = ty < P;
  const typename Src::Column col = src.bind(c0 + (live ? tx : 0));
  const double* e = edges + (int64_t)(c0 + (live ? tx : 0)) * (n_bins + 1);
  const double e0 = e[0], eN = e[n_bins];
  const double scale = (double)n_bins / (eN - e0);
  const int64_t step = (int64_t)gridDim.y * P;
  const int64_t first = (int64_t)blockIdx.y * P;  // the workgroup's first row: the trip count below is a function of it alone
  for (int64_t base = first; base < n_rows; base += step * Src::kUnroll) {
    const int64_t r = base + ty;
    float x[Src::kUnroll];
#pragma unroll
    for (int u = 0; u < Src::kUnroll; ++u) x[u] = live && r + u * step < n_rows ? col.load(r + u * step) : 0.f;
#pragma unroll
    for (int u = 0; u < Src::kUnroll; ++u) {
      bool pending = live && r + u * step < n_rows;
      int slot = 0;
      if (pending) {
        const double xd = (double)x[u];
        int b;
        if (x[u] != x[u]) b = n_bins + 2;
        else if (xd < e0) b = n_bins;
        else if (xd > eN) b = n_bins + 1;
        else b = find_bin(xd, e, n_bins, e0, scale);
        slot = b * W + tx;
      }
      if (AGG) {
        unsigned long long todo = __ballot(pending);
        for (int round = 0; round < kAggRounds && todo; ++round) {
          const int leader = __ffsll((long long)todo) - 1;
          const int s = __shfl(slot, leader);
          const unsigned long long same = __ballot(pending && slot == s);
          if ((int)(tid & 63) == leader) atomicAdd(&hist[s], (unsigned)__popcll(same));
          if (slot == s) pending = false;
          todo &= ~same;
        }
      }
      if (pending) atomicAdd(&hist[slot], 1u);
    }
  }
  __syncthreads();
  for (int s = tid; s < slots; s += kColThreads) {
    const unsigned v = hist[s];
    if (!v) continue;
    const int b = s / W, c = c0 + (s - b * W);
    if (b < n_bins) atomicAdd(&counts[(int64_t)c * n_bins + b], (unsigned long long)v);
    else atomicAdd(&outside[(int64_t)c * 3 + (b - n_bins)], (unsigned long long)v);
  }
}

template <typename Src>
int launch_range(const Src& src, int64_t n_rows, int n_cols, float* out_lo, float* out_hi, int64_t* out_nonfinite, hipStream_t s) {
  const int64_t n_tiles = ((int64_t)n_cols + kRangeTile - 1) / kRangeTile;
  const int W = n_cols < kRangeTile ? n_cols : kRangeTile;
  const int gy = rows_grid(n_rows, W, n_tiles);
  const unsigned cb = (unsigned)((n_cols + 255) / 256);
  hipLaunchKernelGGL(range_init_kernel, dim3(cb), dim3(256), 0, s, (unsigned*)out_lo, (unsigned*)out_hi,
                     (unsigned long long*)out_nonfinite, n_cols);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(range_kernel<Src>, dim3((unsigned)n_tiles, (unsigned)gy), dim3(kColThreads), 0, s, src, n_rows, n_cols,
                     (unsigned*)out_lo, (unsigned*)out_hi, (unsigned long long*)out_nonfinite);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(range_decode_kernel, dim3(cb), dim3(256), 0, s, (unsigned*)out_lo, (unsigned*)out_hi, n_cols);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

template <typename Src>
int launch_histogram(const Src& src, int64_t n_rows, int n_cols, const double* edges, int n_bins, int64_t* counts, int64_t* outside,
                     hipStream_t s) {
  const int tile = hist_tile(n_bins);
  const int64_t n_tiles = ((int64_t)n_cols + tile - 1) / tile;
  const int W = n_cols < tile ? n_cols : tile;  // the widest tile of the launch
  const int gy = rows_grid(n_rows, W, n_tiles);
  const size_t lds = (size_t)(n_bins + 3) * W * sizeof(unsigned);
  // a narrow last tile of a wide launch shares columns between the lanes of a wave as well; it takes the plain atomics, which are
  // correct for any W
  auto kernel = W < 64 ? histogram_kernel<Src, true> : histogram_kernel<Src, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tiles, (unsigned)gy), dim3(kColThreads), lds, s, src, n_rows, n_cols, edges, n_bins, tile,
                     (unsigned long long*)counts, (unsigned long long*)outside);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

// ---- joint histograms --------------------------------------------------------------------------------------------------------------
// A workgroup owns one pair (x column, y column), one band of that pair's [bins_x, bins_y] plane - a run of whole x-rows that fits
// kHistLdsBytes as u32 counters beside the three outside counters - and every gridDim.y-th block of kColThreads rows; lanes are
// consecutive rows.  Every band's workgroups read the rows and count what falls into the band; the outside counters are band 0's.
// LDS: counters [band x-rows][bins_y] u32, then (band 0) x outside / y outside / NaN.  AGG: the wave vote of histogram_kernel, left
// as soon as a round retires fewer than kJointVoteMin lanes.  It is NOT what tw_joint_histogram runs: on a time-ordered trajectory
// whose wells spread over some fifty bins a wave still hits many counters, and plain LDS atomics measured a tenth faster there, on
// shuffled rows and with every row in one bin (profiles/joint_histogram.txt); the vote is reachable as TW_JOINT_PATH_VOTE only.
// The merge is histogram_kernel's.
constexpr int kJointUnroll = 4;
constexpr int kJointVoteMin = 4;
constexpr int64_t kJointMaxPlane = 1ll << 20;

__host__ __device__ inline int joint_band_rows(int bins_x, int bins_y) {
  const int fit = (kHistLdsBytes / 4 - 3) / bins_y;  // bins_y <= TW_HIST_MAX_BINS: at least 3
  return fit > bins_x ? bins_x : fit;
}

inline int joint_bands(int bins_x, int bins_y) {
  const int b = joint_band_rows(bins_x, bins_y);
  return (bins_x + b - 1) / b;
}

// row shares of a (pair, band) unit: rows_grid's budget, and a share reads at least as many rows as its merge walks counters
int joint_row_shares(int64_t n_rows, int64_t units, int counters) {
  const int64_t row_blocks = (n_rows + kColThreads - 1) / kColThreads;
  int64_t want = (kColTargetWgs + units - 1) / units;
  if (want > n_rows / counters) want = n_rows / counters;
  if (want > row_blocks) want = row_blocks;
  return (int)(want < 1 ? 1 : want);
}

template <bool AGG>
__global__ __launch_bounds__(kColThreads) void joint_histogram_kernel(const float* __restrict__ X, int64_t n_rows, int64_t ld,
                                                                      int64_t col_stride, const int* __restrict__ pairs,
                                                                      const double* __restrict__ edges_x, int bins_x,
                                                                      const double* __restrict__ edges_y, int bins_y, int band_rows,
                                                                      int n_bands, unsigned long long* __restrict__ counts,
                                                                      unsigned long long* __restrict__ outside) {
  extern __shared__ unsigned hist[];
  const int p = blockIdx.x / n_bands, band = blockIdx.x - p * n_bands;
  const int x0 = band * band_rows;
  const int x_rows = bins_x - x0 < band_rows ? bins_x - x0 : band_rows;
  const int plane = x_rows * bins_y;
  const bool first_band = band == 0;
  const int slots = plane + (first_band ? 3 : 0);
  const int tid = threadIdx.x;
  for (int s = tid; s < slots; s += kColThreads) hist[s] = 0u;
  __syncthreads();

  const float* px = X + (int64_t)pairs[2 * p] * col_stride;
  const float* py = X + (int64_t)pairs[2 * p + 1] * col_stride;
  const double* ex = edges_x + (int64_t)p * (bins_x + 1);
  const double* ey = edges_y + (int64_t)p * (bins_y + 1);
  const double ex0 = ex[0], exN = ex[bins_x], ey0 = ey[0], eyN = ey[bins_y];
  const double sx = (double)bins_x / (exN - ex0), sy = (double)bins_y / (eyN - ey0);
  const int64_t step = (int64_t)gridDim.y * kColThreads;
  const int64_t first = (int64_t)blockIdx.y * kColThreads;  // the trip count is a function of it alone: the same for every wave
  for (int64_t base = first; base < n_rows; base += step * kJointUnroll) {
    const int64_t r = base + tid;
    float x[kJointUnroll], y[kJointUnroll];
#pragma unroll
    for (int u = 0; u < kJointUnroll; ++u) {
      const bool in = r + u * step < n_rows;
      x[u] = in ? px[(r + u * step) * ld] : 0.f;
      y[u] = in ? py[(r + u * step) * ld] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kJointUnroll; ++u) {
      bool pending = r + u * step < n_rows;
      int slot = 0;
      if (pending) {
        const double xd = (double)x[u], yd = (double)y[u];
        if (x[u] != x[u] || y[u] != y[u]) {
          slot = plane + 2, pending = first_band;
        } else if (xd < ex0 || xd > exN) {
          slot = plane, pending = first_band;
        } else if (yd < ey0 || yd > eyN) {
          slot = plane + 1, pending = first_band;
        } else {
          const int ix = find_bin(xd, ex, bins_x, ex0, sx) - x0;
          if (ix >= 0 && ix < x_rows) slot = ix * bins_y + find_bin(yd, ey, bins_y, ey0, sy);
          else pending = false;
        }
      }
      if (AGG) {
        unsigned long long todo = __ballot(pending);
        for (int round = 0; round < kAggRounds && todo; ++round) {
          const int leader = __ffsll((long long)todo) - 1;
          const int s = __shfl(slot, leader);
          const unsigned long long same = __ballot(pending && slot == s);
          const int n = __popcll(same);
          if ((int)(tid & 63) == leader) atomicAdd(&hist[s], (unsigned)n);
          if (slot == s) pending = false;
          todo &= ~same;
          if (n < kJointVoteMin) break;
        }
      }
      if (pending) atomicAdd(&hist[slot], 1u);
    }
  }
  __syncthreads();
  unsigned long long* plane_out = counts + ((int64_t)p * bins_x + x0) * bins_y;
  for (int s = tid; s < slots; s += kColThreads) {
    const unsigned v = hist[s];
    if (!v) continue;
    if (s < plane) atomicAdd(&plane_out[s], (unsigned long long)v);
    else atomicAdd(&outside[(int64_t)p * 3 + (s - plane)], (unsigned long long)v);
  }
}

}  // namespace
}  // namespace tw

using namespace tw;

int32_t tw_histogram_column_tile(int32_t n_bins) {
  if (n_bins < 1 || n_bins > TW_HIST_MAX_BINS) return -1;
  return hist_tile(n_bins);
}

int tw_pair_distances(const float* coords, const int32_t* pairs, int32_t n_pairs, float* out, int64_t n_rows, int32_t n_atoms,
                      void* stream) {
  TW_REQUIRE(n_pairs >= 0 && n_rows >= 0 && n_atoms > 0, "tw_pair_distances: n_pairs %d, n_rows %lld, n_atoms %d", n_pairs,
             (long long)n_rows, n_atoms);
  TW_REQUIRE(n_pairs <= TW_EVAL_MAX_COLS, "tw_pair_distances: n_pairs %d: at most 2^24", n_pairs);
  if (n_pairs == 0 || n_rows == 0) return TW_OK;  // nothing to compute: no launch
  TW_REQUIRE(coords && pairs && out, "tw_pair_distances: NULL pointer argument");
  const int rpb = n_pairs >= kDistItems ? 1 : kDistItems / n_pairs;
  const int64_t blocks = (n_rows + rpb - 1) / rpb;
  TW_REQUIRE(blocks <= 0x7fffffffll, "tw_pair_distances: n_rows %lld: more than 2^31 - 1 row blocks of %d rows", (long long)n_rows, rpb);
  hipLaunchKernelGGL(pair_distances_kernel, dim3((unsigned)blocks), dim3(kDistThreads), 0, (hipStream_t)stream, coords, pairs, n_pairs,
                     out, n_rows, n_atoms, rpb);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

namespace {

// the refusals the column calls share; `what` names the entry point
int check_columns(const char* what, int64_t n_rows, int64_t n_cols, const char* cols_name) {
  TW_REQUIRE(n_rows >= 0, "%s: n_rows %lld is negative", what, (long long)n_rows);
  TW_REQUIRE(n_cols >= 0, "%s: %s %lld is negative", what, cols_name, (long long)n_cols);
  TW_REQUIRE(n_rows <= kMaxRows, "%s: n_rows %lld: a call takes fewer than 2^32 rows (chunks accumulate)", what, (long long)n_rows);
  TW_REQUIRE(n_cols <= TW_EVAL_MAX_COLS, "%s: %s %lld: at most 2^24", what, cols_name, (long long)n_cols);
  return TW_OK;
}

int check_strided(const char* what, int64_t n_cols, int64_t ld, int64_t col_stride) {
  TW_REQUIRE(col_stride >= 1, "%s: col_stride %lld: at least 1", what, (long long)col_stride);
  // (n_cols - 1) col_stride + 1 below must not wrap: n_cols <= 2^24, so col_stride <= 2^38 keeps it under 2^62
  TW_REQUIRE(col_stride <= (1ll << 38), "%s: col_stride %lld: at most 2^38", what, (long long)col_stride);
  TW_REQUIRE(n_cols == 0 || ld >= (n_cols - 1) * col_stride + 1, "%s: ld %lld: a row of %lld columns %lld apart takes %lld", what,
             (long long)ld, (long long)n_cols, (long long)col_stride, (long long)((n_cols - 1) * col_stride + 1));
  return TW_OK;
}

int check_bins(const char* what, int32_t n_bins, int64_t n_cols) {
  TW_REQUIRE(n_bins >= 1 && n_bins <= TW_HIST_MAX_BINS, "%s: n_bins %d: 1 .. %d", what, n_bins, TW_HIST_MAX_BINS);
  const int tile = hist_tile(n_bins);
  TW_REQUIRE((n_cols + tile - 1) / tile <= kMaxTiles, "%s: %lld columns in tiles of %d: more than 2^20 column tiles", what,
             (long long)n_cols, tile);
  return TW_OK;
}

}  // namespace

int tw_column_range(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, float* out_lo, float* out_hi,
                    int64_t* out_nonfinite, void* stream) {
  if (int rc = check_columns("tw_column_range", n_rows, n_cols, "n_cols")) return rc;
  if (int rc = check_strided("tw_column_range", n_cols, ld, col_stride)) return rc;
  if (n_rows == 0 || n_cols == 0) return TW_OK;  // nothing to read: no launch
  TW_REQUIRE(X && out_lo && out_hi && out_nonfinite, "tw_column_range: NULL pointer argument");
  return launch_range(StridedSource{X, ld, col_stride}, n_rows, n_cols, out_lo, out_hi, out_nonfinite, (hipStream_t)stream);
}

int tw_column_histogram(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const double* edges,
                        int32_t n_bins, int64_t* counts, int64_t* outside, void* stream) {
  if (int rc = check_columns("tw_column_histogram", n_rows, n_cols, "n_cols")) return rc;
  if (int rc = check_strided("tw_column_histogram", n_cols, ld, col_stride)) return rc;
  if (int rc = check_bins("tw_column_histogram", n_bins, n_cols)) return rc;
  if (n_rows == 0 || n_cols == 0) return TW_OK;  // nothing to count: no launch
  TW_REQUIRE(X && edges && counts && outside, "tw_column_histogram: NULL pointer argument");
  return launch_histogram(StridedSource{X, ld, col_stride}, n_rows, n_cols, edges, n_bins, counts, outside, (hipStream_t)stream);
}

int tw_pair_range(const float* coords, const int32_t* pairs, int32_t n_pairs, int64_t n_rows, int32_t n_atoms, float* out_lo,
                  float* out_hi, int64_t* out_nonfinite, void* stream) {
  if (int rc = check_columns("tw_pair_range", n_rows, n_pairs, "n_pairs")) return rc;
  TW_REQUIRE(n_atoms > 0, "tw_pair_range: n_atoms %d: at least 1", n_atoms);
  if (n_rows == 0 || n_pairs == 0) return TW_OK;  // nothing to read: no launch
  TW_REQUIRE(coords && pairs && out_lo && out_hi && out_nonfinite, "tw_pair_range: NULL pointer argument");
  return launch_range(PairSource{coords, pairs, n_atoms}, n_rows, n_pairs, out_lo, out_hi, out_nonfinite, (hipStream_t)stream);
}

int tw_pair_histogram(const float* coords, const int32_t* pairs, int32_t n_pairs, int64_t n_rows, int32_t n_atoms, const double* edges,
                      int32_t n_bins, int64_t* counts, int64_t* outside, void* stream) {
  if (int rc = check_columns("tw_pair_histogram", n_rows, n_pairs, "n_pairs")) return rc;
  TW_REQUIRE(n_atoms > 0, "tw_pair_histogram: n_atoms %d: at least 1", n_atoms);
  if (int rc = check_bins("tw_pair_histogram", n_bins, n_pairs)) return rc;
  if (n_rows == 0 || n_pairs == 0) return TW_OK;  // nothing to count: no launch
  TW_REQUIRE(coords && pairs && edges && counts && outside, "tw_pair_histogram: NULL pointer argument");
  return launch_histogram(PairSource{coords, pairs, n_atoms}, n_rows, n_pairs, edges, n_bins, counts, outside, (hipStream_t)stream);
}

int32_t tw_joint_histogram_bands(int32_t bins_x, int32_t bins_y) {
  if (bins_x < 1 || bins_x > TW_HIST_MAX_BINS || bins_y < 1 || bins_y > TW_HIST_MAX_BINS) return -1;
  if ((int64_t)bins_x * bins_y > kJointMaxPlane) return -1;
  return joint_bands(bins_x, bins_y);
}

int tw_joint_histogram_path(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const int32_t* pairs,
                            int32_t n_pairs, const double* edges_x, int32_t bins_x, const double* edges_y, int32_t bins_y,
                            int64_t* counts, int64_t* outside, int32_t path, void* stream) {
  const char* what = "tw_joint_histogram";
  if (int rc = check_columns(what, n_rows, n_pairs, "n_pairs")) return rc;
  TW_REQUIRE(n_cols >= 0 && n_cols <= TW_EVAL_MAX_COLS, "%s: n_cols %d: 0 .. 2^24", what, n_cols);
  if (int rc = check_strided(what, n_cols, ld, col_stride)) return rc;
  TW_REQUIRE(bins_x >= 1 && bins_x <= TW_HIST_MAX_BINS, "%s: bins_x %d: 1 .. %d", what, bins_x, TW_HIST_MAX_BINS);
  TW_REQUIRE(bins_y >= 1 && bins_y <= TW_HIST_MAX_BINS, "%s: bins_y %d: 1 .. %d", what, bins_y, TW_HIST_MAX_BINS);
  TW_REQUIRE((int64_t)bins_x * bins_y <= kJointMaxPlane, "%s: bins_x %d times bins_y %d: a plane holds at most 2^20 bins", what, bins_x,
             bins_y);
  TW_REQUIRE(path == TW_JOINT_PATH_AUTO || path == TW_JOINT_PATH_PLAIN || path == TW_JOINT_PATH_VOTE, "%s: path %d: 0, 1 or 2", what,
             path);
  if (n_rows == 0 || n_pairs == 0) return TW_OK;  // nothing to count: no launch
  TW_REQUIRE(n_cols >= 1, "%s: n_cols 0: the pairs name columns 0 .. n_cols - 1", what);
  TW_REQUIRE(X && pairs && edges_x && edges_y && counts && outside, "%s: NULL pointer argument", what);
  const int band_rows = joint_band_rows(bins_x, bins_y);
  const int n_bands = joint_bands(bins_x, bins_y);
  const int64_t units = (int64_t)n_pairs * n_bands;  // at most 2^24 pairs of at most 86 bands: below 2^31
  TW_REQUIRE(units <= 0x7fffffffll, "%s: n_pairs %d of %d bands: more than 2^31 - 1 workgroup columns", what, n_pairs, n_bands);
  const int gy = joint_row_shares(n_rows, units, band_rows * bins_y);
  const size_t lds = ((size_t)band_rows * bins_y + 3) * sizeof(unsigned);
  // measured (profiles/joint_histogram.txt): the vote costs a tenth at 100 x 100 whatever the order of the rows
  auto kernel = path == TW_JOINT_PATH_VOTE ? joint_histogram_kernel<true> : joint_histogram_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)units, (unsigned)gy), dim3(kColThreads), lds, (hipStream_t)stream, X, n_rows, ld, col_stride,
                     pairs, edges_x, bins_x, edges_y, bins_y, band_rows, n_bands, (unsigned long long*)counts,
                     (unsigned long long*)outside);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int tw_joint_histogram(const float* X, int64_t n_rows, int32_t n_cols, int64_t ld, int64_t col_stride, const int32_t* pairs,
                       int32_t n_pairs, const double* edges_x, int32_t bins_x, const double* edges_y, int32_t bins_y, int64_t* counts,
                       int64_t* outside, void* stream) {
  return tw_joint_histogram_path(X, n_rows, n_cols, ld, col_stride, pairs, n_pairs, edges_x, bins_x, edges_y, bins_y, counts, outside,
                                 TW_JOINT_PATH_AUTO, stream);
}
