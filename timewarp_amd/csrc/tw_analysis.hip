// Trajectory analysis on the device (timewarp_amd/analysis.py): torsion angles, the TICA feature vector and the time-lagged second
// moments the TICA estimator is built from.  The entry points are declared in include/timewarp_hip.h, which also states what each
// computes; this file holds the kernels and the argument checks.
#include "tw_common.h"

namespace tw {
namespace {

// ---- featurisation ---------------------------------------------------------------------------------------------------------------
// One workgroup stages the coordinates of a block of rows into LDS (one coalesced pass over rows * n_atoms * 3 floats) and its threads
// then walk the (row, output column) items of that block, so consecutive threads store consecutive floats of `out`.
constexpr int kFeatThreads = 256;
constexpr int kFeatMaxRows = 64;          // rows per workgroup, fewer when the molecule is large
constexpr int kFeatLdsBytes = 64 * 1024;  // the dynamic LDS a launch gets without opting in

struct Torsion {
  double y, x;  // angle = atan2(y, x)
};

// mdtraj's convention: b1 = x1-x0, b2 = x2-x1, b3 = x3-x2, c1 = b2 x b3, c2 = b1 x b2, angle = atan2((b1.c1) |b2|, c1.c2).
// fp64 from the float32 coordinates: the caller rounds once.
__device__ __forceinline__ Torsion torsion_xy(const float* xs, const int* quad) {
  double p[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* s = xs + 3 * quad[a];
    p[a][0] = (double)s[0], p[a][1] = (double)s[1], p[a][2] = (double)s[2];
  }
  double b1[3], b2[3], b3[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) b1[d] = p[1][d] - p[0][d], b2[d] = p[2][d] - p[1][d], b3[d] = p[3][d] - p[2][d];
  const double c1[3] = {b2[1] * b3[2] - b2[2] * b3[1], b2[2] * b3[0] - b2[0] * b3[2], b2[0] * b3[1] - b2[1] * b3[0]};
  const double c2[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
  const double nb2 = sqrt(b2[0] * b2[0] + b2[1] * b2[1] + b2[2] * b2[2]);
  Torsion t;
  t.y = (b1[0] * c1[0] + b1[1] * c1[1] + b1[2] * c1[2]) * nb2;
  t.x = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2];
  return t;
}

__device__ __forceinline__ void stage_rows(const float* coords, int64_t row0, int rows, int n_atoms, float* xs) {
  const int64_t n = (int64_t)rows * n_atoms * 3;
  const float* src = coords + row0 * n_atoms * 3;
  for (int64_t i = threadIdx.x; i < n; i += kFeatThreads) xs[i] = src[i];
  __syncthreads();
}

__global__ __launch_bounds__(kFeatThreads) void dihedrals_kernel(const float* __restrict__ coords, const int* __restrict__ quads,
                                                                 int n_quads, float* __restrict__ out, int64_t n_rows, int n_atoms,
                                                                 int rows_per_block) {
  extern __shared__ float xs[];
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int rows = (int)(n_rows - row0 < rows_per_block ? n_rows - row0 : rows_per_block);
  stage_rows(coords, row0, rows, n_atoms, xs);
  const int items = rows * n_quads;
  for (int it = threadIdx.x; it < items; it += kFeatThreads) {
    const int r = it / n_quads, q = it - r * n_quads;
    int quad[4] = {quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q + 3]};
    const Torsion t = torsion_xy(xs + (size_t)r * n_atoms * 3, quad);
    out[row0 * n_quads + it] = (float)atan2(t.y, t.x);  // atan2(0, 0) = 0: a collinear quad
  }
}

// Column k of the distance block is the pair (i, j), i < j, in np.triu_indices(n, k=1) order: k = i n - i (i + 1) / 2 + j - i - 1.
__device__ __forceinline__ void triu_pair(int k, int n, int* pi, int* pj) {
  const double disc = (double)(2 * n - 1) * (double)(2 * n - 1) - 8.0 * (double)k;
  int i = (int)(((double)(2 * n - 1) - sqrt(disc)) * 0.5);
  i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
  // first column of row i: i (2n - i - 1) / 2
  while (i > 0 && (int64_t)i * (2 * n - i - 1) / 2 > k) --i;
  while (i < n - 2 && (int64_t)(i + 1) * (2 * n - i - 2) / 2 <= k) ++i;
  *pi = i;
  *pj = k - (int)((int64_t)i * (2 * n - i - 1) / 2) + i + 1;
}

__global__ __launch_bounds__(kFeatThreads) void tica_features_kernel(const float* __restrict__ coords, const int* __restrict__ atom_sel,
                                                                     int n_sel, const int* __restrict__ quads,
                                                                     const int* __restrict__ quad_cols, int n_quads,
                                                                     float* __restrict__ out, int64_t n_rows, int n_atoms,
                                                                     int rows_per_block) {
  extern __shared__ float xs[];
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int rows = (int)(n_rows - row0 < rows_per_block ? n_rows - row0 : rows_per_block);
  stage_rows(coords, row0, rows, n_atoms, xs);
  const int n_pairs = n_sel > 1 ? n_sel * (n_sel - 1) / 2 : 0;
  const int F = n_pairs + 2 * n_quads;
  if (n_pairs > 0) {
    const int items = rows * n_pairs;
    for (int it = threadIdx.x; it < items; it += kFeatThreads) {
      const int r = it / n_pairs, k = it - r * n_pairs;
      int i, j;
      triu_pair(k, n_sel, &i, &j);
      const float* a = xs + ((size_t)r * n_atoms + atom_sel[i]) * 3;
      const float* b = xs + ((size_t)r * n_atoms + atom_sel[j]) * 3;
      const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
      out[(row0 + r) * F + k] = (float)sqrt(dx * dx + dy * dy + dz * dz);
    }
  }
  const int items = rows * n_quads;
  for (int it = threadIdx.x; it < items; it += kFeatThreads) {
    const int r = it / n_quads, q = it - r * n_quads;
    int quad[4] = {quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q + 3]};
    const Torsion t = torsion_xy(xs + (size_t)r * n_atoms * 3, quad);
    // sin and cos of atan2(y, x) without the angle: (y, x) / |(y, x)|, and (0, 1) for the collinear quad whose angle is 0
    const double h = sqrt(t.y * t.y + t.x * t.x);
    const double s = h == 0.0 ? 0.0 : t.y / h, c = h == 0.0 ? 1.0 : t.x / h;
    float* o = out + (row0 + r) * F + n_pairs;
    o[quad_cols[2 * q]] = (float)s;
    o[quad_cols[2 * q + 1]] = (float)c;
  }
}

int feature_rows_per_block(int n_atoms) {
  const int fit = kFeatLdsBytes / (n_atoms * 3 * (int)sizeof(float));
  return fit > kFeatMaxRows ? kFeatMaxRows : fit;
}

// ---- lagged second moments -------------------------------------------------------------------------------------------------------
// C = sum over pairs of a b^T for (a, b) = (x, y), (x, x), (y, y): a tall-skinny product.  The output is cut into 128 x 128 tiles; of
// the two symmetric matrices only the tiles on and above the diagonal are computed.  The pair axis (all chains' pairs, chain after
// chain) is cut into `n_splits` equal contiguous ranges.  One workgroup of four waves computes one tile over one range on the fp64 MFMA
// (v_mfma_f64_16x16x4_f64; each wave owns a 64 x 64 quadrant = 4 x 4 accumulators of 4 doubles), from chunks of 16 frames staged
// through LDS as fp64, and writes its partial tile to the workspace.  reduce_kernel then adds the partials of every entry in range
// order into the caller's accumulators.  Nothing is atomic, the split is a function of the shapes alone: a call is bit-reproducible.
constexpr int kTile = 128;           // features per tile edge
constexpr int kChunk = 16;           // frames staged per step
constexpr int kStride = kTile + 16;  // doubles per staged frame: 288 dwords = 32 mod 64, two k rows of a half wave hit disjoint banks
constexpr int kMomThreads = 256;
constexpr int kMaxSplits = 128;
constexpr int kTargetBlocks = 1024;  // ~2 rounds of 2 workgroups on each of 256 CUs

typedef double double4_t __attribute__((ext_vector_type(4)));

struct MomentsPlan {
  int nt;        // tiles per edge
  int n_tri;     // nt (nt + 1) / 2
  int n_jobs;    // nt^2 + 2 n_tri
  int n_splits;  // for the largest pair count (the workspace is sized by it)
};

MomentsPlan moments_plan(int F) {
  MomentsPlan p;
  p.nt = (F + kTile - 1) / kTile;
  p.n_tri = p.nt * (p.nt + 1) / 2;
  p.n_jobs = p.nt * p.nt + 2 * p.n_tri;
  int s = kTargetBlocks / p.n_jobs;
  p.n_splits = s < 1 ? 1 : (s > kMaxSplits ? kMaxSplits : s);
  return p;
}

int64_t moments_workspace_len(int F) {
  const MomentsPlan p = moments_plan(F);
  return (int64_t)p.n_splits * ((int64_t)p.n_jobs * kTile * kTile + 2 * (int64_t)F);
}

// job -> (matrix m: 0 = xy, 1 = xx, 2 = yy; tile row ti; tile column tj).  The triangular jobs are numbered row after row, tj >= ti.
__device__ __forceinline__ void decode_job(int job, int nt, int n_tri, int* m, int* ti, int* tj) {
  if (job < nt * nt) {
    *m = 0, *ti = job / nt, *tj = job - (job / nt) * nt;
    return;
  }
  job -= nt * nt;
  *m = 1 + job / n_tri;
  job -= (job / n_tri) * n_tri;
  int i = 0;
  while (job >= nt - i) job -= nt - i, ++i;
  *ti = i, *tj = i + job;
}

// frame index (row of X) of pair p: pairs never cross a chain, chain c owns pairs c P .. c P + P - 1 and frames c T .. c T + T - 1
__device__ __forceinline__ int64_t pair_frame(uint32_t p, uint32_t P, int T) {
  const uint32_t c = p / P;
  return (int64_t)c * T + (p - c * P);
}

// WEIGHTED: the pair's weight W[frame of x] multiplies the a operand as it is staged, rnd((double)a w) - one rounding more per term;
// with w = 1.0 the product is exact and the kernel computes what the unweighted one does, bit for bit.
template <bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(kMomThreads, 2) void moments_tile_kernel(const float* __restrict__ X, const double* __restrict__ W, int T,
                                                                      int F, int lag, uint32_t P, uint32_t n_pairs, int n_splits,
                                                                      int nt, int n_tri, int n_jobs, double* __restrict__ ws) {
  __shared__ double As[kChunk * kStride];
  __shared__ double Bs[kChunk * kStride];
  int m, ti, tj;
  decode_job(blockIdx.x, nt, n_tri, &m, &ti, &tj);
  const int split = blockIdx.y;
  const uint32_t per = (n_pairs + n_splits - 1) / n_splits;
  const uint32_t p0 = (uint32_t)split * per < n_pairs ? (uint32_t)split * per : n_pairs;
  const uint32_t p1 = n_pairs - p0 < per ? n_pairs : p0 + per;
  const int a_off = m == 2 ? lag : 0, b_off = m == 1 ? 0 : lag;  // x frames for a / b, or the y frames `lag` later
  const int fa0 = ti * kTile, fb0 = tj * kTile;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  double4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  // what this thread stages of a chunk: VEC - float4 number tid and tid + 256 of the 16 x 32 float4s of each operand; otherwise
  // feature tid & 127 of the frames (tid >> 7) + 2 r
  constexpr int NV = VEC ? 2 : 8;
  float4 ra[VEC ? 2 : 1], rb[VEC ? 2 : 1];
  float sa[VEC ? 1 : 8], sb[VEC ? 1 : 8];
  double wv[WEIGHTED ? NV : 1];

  auto fetch = [&](uint32_t pc) {
#pragma unroll
    for (int r = 0; r < NV; ++r) {
      const int k = VEC ? (tid + 256 * r) >> 5 : (tid >> 7) + 2 * r;
      const int f = VEC ? ((tid + 256 * r) & 31) * 4 : tid & 127;
      const bool live = pc + k < p1;
      const int64_t frame = live ? pair_frame(pc + k, P, T) : 0;
      if (WEIGHTED) wv[r] = live ? W[frame] : 0.0;
      if (VEC) {
        ra[r] = live && fa0 + f < F ? *(const float4*)(X + (frame + a_off) * F + fa0 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
        rb[r] = live && fb0 + f < F ? *(const float4*)(X + (frame + b_off) * F + fb0 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        sa[r] = live && fa0 + f < F ? X[(frame + a_off) * F + fa0 + f] : 0.f;
        sb[r] = live && fb0 + f < F ? X[(frame + b_off) * F + fb0 + f] : 0.f;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int r = 0; r < NV; ++r) {
      const int k = VEC ? (tid + 256 * r) >> 5 : (tid >> 7) + 2 * r;
      const int f = VEC ? ((tid + 256 * r) & 31) * 4 : tid & 127;
      if (VEC) {
        double* a = As + k * kStride + f;
        double* b = Bs + k * kStride + f;
        if (WEIGHTED)
          a[0] = (double)ra[r].x * wv[r], a[1] = (double)ra[r].y * wv[r], a[2] = (double)ra[r].z * wv[r], a[3] = (double)ra[r].w * wv[r];
        else
          a[0] = (double)ra[r].x, a[1] = (double)ra[r].y, a[2] = (double)ra[r].z, a[3] = (double)ra[r].w;
        b[0] = (double)rb[r].x, b[1] = (double)rb[r].y, b[2] = (double)rb[r].z, b[3] = (double)rb[r].w;
      } else {
        As[k * kStride + f] = WEIGHTED ? (double)sa[r] * wv[r] : (double)sa[r];
        Bs[k * kStride + f] = (double)sb[r];
      }
    }
  };

  if (p0 < p1) fetch(p0);
  for (uint32_t pc = p0; pc < p1; pc += kChunk) {
    __syncthreads();  // the previous chunk has been read
    stage();
    __syncthreads();
    if (pc + kChunk < p1) fetch(pc + kChunk);  // in flight while this chunk is multiplied
#pragma unroll
    for (int k0 = 0; k0 < kChunk; k0 += 4) {
      // operand maps of the 16x16x4 form: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15]
      const double* ap = As + (k0 + (lane >> 4)) * kStride + wr + (lane & 15);
      const double* bp = Bs + (k0 + (lane >> 4)) * kStride + wc + (lane & 15);
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = ap[16 * i], b[i] = bp[16 * i];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D map of the f64 form: register r of lane l is row (l >> 4) + 4 r, column l & 15
  double* tile = ws + ((int64_t)split * n_jobs + blockIdx.x) * (kTile * kTile);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tile[(wr + 16 * i + (lane >> 4) + 4 * r) * kTile + wc + 16 * j + (lane & 15)] = acc[i][j][r];
}

// partial sums of x and y per split: thread (feature f, slot s of 4) adds its range's pairs s, s + 4, ... in that order; the four slots
// are then added in slot order.  WEIGHTED: each term is rnd((double)x w), rounded before it is added (no contraction into an fma).
template <bool WEIGHTED>
__global__ __launch_bounds__(kMomThreads) void moments_sums_kernel(const float* __restrict__ X, const double* __restrict__ W, int T, int F,
                                                                   int lag, uint32_t P, uint32_t n_pairs, int n_splits,
                                                                   double* __restrict__ sums) {
  __shared__ double part[2][4][64];
  const int split = blockIdx.y, fl = threadIdx.x & 63, slot = threadIdx.x >> 6, f = blockIdx.x * 64 + fl;
  const uint32_t per = (n_pairs + n_splits - 1) / n_splits;
  const uint32_t p0 = (uint32_t)split * per < n_pairs ? (uint32_t)split * per : n_pairs;
  const uint32_t p1 = n_pairs - p0 < per ? n_pairs : p0 + per;
  double sx = 0.0, sy = 0.0;
  if (f < F)
    for (uint32_t p = p0 + slot; p < p1; p += 4) {
      const int64_t frame = pair_frame(p, P, T);
      if (WEIGHTED) {
        const double w = W[frame];
        sx += __dmul_rn((double)X[frame * F + f], w);
        sy += __dmul_rn((double)X[(frame + lag) * F + f], w);
      } else {
        sx += (double)X[frame * F + f];
        sy += (double)X[(frame + lag) * F + f];
      }
    }
  part[0][slot][fl] = sx, part[1][slot][fl] = sy;
  __syncthreads();
  if (slot < 2 && f < F)
    sums[((int64_t)split * 2 + slot) * F + f] = ((part[slot][0][fl] + part[slot][1][fl]) + part[slot][2][fl]) + part[slot][3][fl];
}

// acc = [sum x (F), sum y (F), Cxx (F^2), Cxy (F^2), Cyy (F^2)]: one thread per entry adds the splits' partials in split order
__global__ __launch_bounds__(256) void moments_reduce_kernel(const double* __restrict__ ws, const double* __restrict__ sums, int F,
                                                             int n_splits, int nt, int n_tri, int n_jobs, double* __restrict__ acc,
                                                             int64_t* __restrict__ n_pairs_out, int64_t n_pairs) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t FF = (int64_t)F * F;
  if (idx == 0 && n_pairs_out) *n_pairs_out += n_pairs;
  if (idx < 2 * (int64_t)F) {
    double s = 0.0;
    for (int k = 0; k < n_splits; ++k) s += sums[(int64_t)k * 2 * F + idx];
    acc[idx] += s;
    return;
  }
  const int64_t e = idx - 2 * (int64_t)F;
  if (e >= 3 * FF) return;
  const int mat = (int)(e / FF);  // 0 = xx, 1 = xy, 2 = yy, the order of `acc`
  int i = (int)((e - mat * FF) / F), j = (int)((e - mat * FF) - (int64_t)i * F);
  int job;
  if (mat == 1) {
    job = (i / kTile) * nt + j / kTile;
  } else {
    if (i / kTile > j / kTile) {  // below the diagonal tiles: the mirrored entry (the same products in the same order)
      const int t = i;
      i = j, j = t;
    }
    const int ti = i / kTile, tj = j / kTile;
    job = nt * nt + (mat == 2 ? n_tri : 0) + ti * nt - ti * (ti - 1) / 2 + (tj - ti);
  }
  const double* src = ws + (int64_t)job * (kTile * kTile) + (i % kTile) * kTile + (j % kTile);
  double s = 0.0;
  for (int k = 0; k < n_splits; ++k) s += src[(int64_t)k * n_jobs * (kTile * kTile)];
  acc[idx] += s;
}

// sum of the pairs' weights, in two launches after the tiles' partials have been consumed (the workspace is free again): the pair axis
// is cut into `nb` contiguous ranges, block i adds its range (thread t the pairs t, t + 256, ... in that order, then a tree over the
// 256 threads) into part[i]; one block then adds part[0 .. nb) by the same tree into *sum_w_out.  The order is a function of n_pairs.
constexpr int kWsumThreads = 256;
constexpr int kWsumMaxBlocks = 256;

__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kWsumThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(kWsumThreads) void weights_partial_kernel(const double* __restrict__ W, int T, uint32_t P, uint32_t n_pairs,
                                                                       double* __restrict__ part) {
  __shared__ double red[kWsumThreads];
  const uint32_t per = (n_pairs + gridDim.x - 1) / gridDim.x;
  const uint32_t p0 = blockIdx.x * per < n_pairs ? blockIdx.x * per : n_pairs;
  const uint32_t p1 = n_pairs - p0 < per ? n_pairs : p0 + per;
  double s = 0.0;
  for (uint32_t p = p0 + threadIdx.x; p < p1; p += kWsumThreads) s += W[pair_frame(p, P, T)];
  s = block_tree_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kWsumThreads) void weights_total_kernel(const double* __restrict__ part, int nb, double* __restrict__ sum_w_out) {
  __shared__ double red[kWsumThreads];
  const double s = block_tree_sum((int)threadIdx.x < nb ? part[threadIdx.x] : 0.0, red);
  if (threadIdx.x == 0) *sum_w_out += s;
}

// ---- projection ------------------------------------------------------------------------------------------------------------------
// out[n, j] = b[j] + sum_f (X[n, f] - m[f]) P[f, j].  One workgroup owns 64 rows and walks F in slices of 64 features: the slice of P
// ([64, k] fp64, at most 32 KiB), of m and the 64 x 64 float32 block of X are staged in LDS (X rows 65 floats apart: the 64 lanes of a
// wave read 64 different rows of one column, 65 is odd, so they hit 64 different banks; P and m are read at one address by a whole
// wave - a broadcast).  Lane l of wave g owns row l and the columns g kc .. g kc + kc - 1, kc = ceil(k / 4) <= 16, each in a register
// that starts at b[j] and takes one fma per feature in ascending order: a row's result depends on nothing but that row.
constexpr int kProjThreads = 256;
constexpr int kProjRows = 64;
constexpr int kProjSlice = 64;
constexpr int kProjXStride = kProjSlice + 1;
constexpr int kProjMaxK = 64;
constexpr int kProjCols = kProjMaxK / (kProjThreads / kProjRows);  // 16 columns per thread at most

size_t project_lds_bytes(int k) { return (size_t)kProjSlice * (k + 1) * sizeof(double) + (size_t)kProjRows * kProjXStride * sizeof(float); }

__global__ __launch_bounds__(kProjThreads) void project_kernel(const float* __restrict__ X, const double* __restrict__ m,
                                                               const double* __restrict__ Pm, const double* __restrict__ b,
                                                               double* __restrict__ out, int64_t n_rows, int F, int k, int kc) {
  extern __shared__ double proj_lds[];
  double* Ps = proj_lds;                            // [kProjSlice][k]
  double* ms = Ps + kProjSlice * k;                 // [kProjSlice]
  float* Xs = (float*)(ms + kProjSlice);            // [kProjRows][kProjXStride]
  const int64_t row0 = (int64_t)blockIdx.x * kProjRows;
  const int rows = (int)(n_rows - row0 < kProjRows ? n_rows - row0 : kProjRows);
  const int tid = threadIdx.x, r = tid & (kProjRows - 1), j0 = (tid / kProjRows) * kc;
  const int nc = k - j0 < kc ? (k - j0 < 0 ? 0 : k - j0) : kc;  // this wave's columns: j0 .. j0 + nc - 1
  double acc[kProjCols];
#pragma unroll
  for (int c = 0; c < kProjCols; ++c) acc[c] = (c < nc && b) ? b[j0 + c] : 0.0;
  for (int f0 = 0; f0 < F; f0 += kProjSlice) {
    const int fs = F - f0 < kProjSlice ? F - f0 : kProjSlice;
    __syncthreads();  // the previous slice has been read
    for (int i = tid; i < fs * k; i += kProjThreads) Ps[i] = Pm[(int64_t)f0 * k + i];  // rows f0 .. f0 + fs - 1 of P are contiguous
    if (tid < fs) ms[tid] = m ? m[f0 + tid] : 0.0;
    for (int i = tid; i < rows * kProjSlice; i += kProjThreads) {
      const int rr = i / kProjSlice, ff = i % kProjSlice;
      if (ff < fs) Xs[rr * kProjXStride + ff] = X[(row0 + rr) * F + f0 + ff];
    }
    __syncthreads();
    if (r < rows && nc > 0)
      for (int ff = 0; ff < fs; ++ff) {
        const double d = (double)Xs[r * kProjXStride + ff] - ms[ff];
        const double* pr = Ps + ff * k + j0;
#pragma unroll
        for (int c = 0; c < kProjCols; ++c)
          if (c < nc) acc[c] = fma(d, pr[c], acc[c]);
      }
  }
  if (r < rows)
#pragma unroll
    for (int c = 0; c < kProjCols; ++c)
      if (c < nc) out[(row0 + r) * k + j0 + c] = acc[c];
}

}  // namespace
}  // namespace tw

using namespace tw;

int tw_dihedrals(const float* coords, const int32_t* quads, int32_t n_quads, float* out, int64_t n_rows, int32_t n_atoms, void* stream) {
  TW_REQUIRE(n_quads >= 0 && n_rows >= 0 && n_atoms > 0, "tw_dihedrals: n_quads %d, n_rows %lld, n_atoms %d", n_quads, (long long)n_rows,
             n_atoms);
  if (n_quads == 0 || n_rows == 0) return TW_OK;  // nothing to compute: no launch
  TW_REQUIRE(coords && quads && out, "NULL pointer argument");
  const int rpb = feature_rows_per_block(n_atoms);
  TW_REQUIRE(rpb >= 1, "n_atoms %d: one row of coordinates must fit %d bytes of LDS", n_atoms, kFeatLdsBytes);
  TW_REQUIRE(n_quads <= (1 << 20), "n_quads %d: at most 2^20", n_quads);
  const int64_t blocks = (n_rows + rpb - 1) / rpb;
  TW_REQUIRE(blocks <= 0x7fffffffll, "n_rows %lld: too many row blocks", (long long)n_rows);
  const size_t lds = (size_t)rpb * n_atoms * 3 * sizeof(float);
  hipLaunchKernelGGL(dihedrals_kernel, dim3((unsigned)blocks), dim3(kFeatThreads), lds, (hipStream_t)stream, coords, quads, n_quads, out,
                     n_rows, n_atoms, rpb);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int tw_tica_features(const float* coords, const int32_t* atom_sel, int32_t n_sel, const int32_t* quads, const int32_t* quad_cols,
                     int32_t n_quads, float* out, int64_t n_rows, int32_t n_atoms, int32_t n_features, void* stream) {
  TW_REQUIRE(n_sel >= 0 && n_quads >= 0 && n_rows >= 0 && n_atoms > 0, "tw_tica_features: n_sel %d, n_quads %d, n_rows %lld, n_atoms %d",
             n_sel, n_quads, (long long)n_rows, n_atoms);
  TW_REQUIRE(n_sel <= 4096 && n_quads <= (1 << 20), "n_sel %d (at most 4096), n_quads %d (at most 2^20)", n_sel, n_quads);
  const int64_t n_pairs = n_sel > 1 ? (int64_t)n_sel * (n_sel - 1) / 2 : 0;
  TW_REQUIRE((int64_t)n_features == n_pairs + 2 * (int64_t)n_quads, "n_features %d: n_sel (n_sel - 1) / 2 + 2 n_quads = %lld", n_features,
             (long long)(n_pairs + 2 * (int64_t)n_quads));
  if (n_features == 0 || n_rows == 0) return TW_OK;  // nothing to compute: no launch
  TW_REQUIRE(coords && out && (n_pairs == 0 || atom_sel) && (n_quads == 0 || (quads && quad_cols)), "NULL pointer argument");
  const int rpb = feature_rows_per_block(n_atoms);
  TW_REQUIRE(rpb >= 1, "n_atoms %d: one row of coordinates must fit %d bytes of LDS", n_atoms, kFeatLdsBytes);
  TW_REQUIRE((int64_t)rpb * n_pairs <= 0x7fffffffll, "n_sel %d: too many pairs per row block", n_sel);
  const int64_t blocks = (n_rows + rpb - 1) / rpb;
  TW_REQUIRE(blocks <= 0x7fffffffll, "n_rows %lld: too many row blocks", (long long)n_rows);
  const size_t lds = (size_t)rpb * n_atoms * 3 * sizeof(float);
  hipLaunchKernelGGL(tica_features_kernel, dim3((unsigned)blocks), dim3(kFeatThreads), lds, (hipStream_t)stream, coords, atom_sel, n_sel,
                     quads, quad_cols, n_quads, out, n_rows, n_atoms, rpb);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int64_t tw_lagged_moments_workspace_len(int32_t n_features) {
  if (n_features < 1 || n_features > TW_MOMENTS_MAX_FEATURES) return -1;
  return moments_workspace_len(n_features);
}

namespace {

int lagged_moments_launch(const float* X, const double* weights, bool weighted, int64_t n_chains, int64_t n_frames, int32_t n_features,
                          int64_t lag, double* acc, int64_t* n_pairs_out, double* sum_w_out, double* workspace, void* stream) {
  TW_REQUIRE(n_features >= 1 && n_features <= TW_MOMENTS_MAX_FEATURES, "n_features %d: 1 .. %d", n_features, TW_MOMENTS_MAX_FEATURES);
  TW_REQUIRE(n_chains >= 0 && n_frames >= 1, "n_chains %lld, n_frames %lld", (long long)n_chains, (long long)n_frames);
  TW_REQUIRE(lag >= 1 && lag < n_frames, "lag %lld: 1 .. n_frames - 1 = %lld (a pair is two frames of one chain)", (long long)lag,
             (long long)n_frames - 1);
  TW_REQUIRE(n_chains * n_frames <= 0x7fffffffll, "n_chains x n_frames = %lld: at most 2^31 - 1 frames per call",
             (long long)(n_chains * n_frames));
  if (n_chains == 0) return TW_OK;  // no pairs: no launch
  TW_REQUIRE(X && acc && workspace, "NULL pointer argument");
  TW_REQUIRE(!weighted || weights, "NULL weights");
  const int F = n_features, T = (int)n_frames;
  const uint32_t P = (uint32_t)(n_frames - lag), n_pairs = (uint32_t)n_chains * P;
  const MomentsPlan plan = moments_plan(F);
  const int64_t chunks = ((int64_t)n_pairs + kChunk - 1) / kChunk;
  const int n_splits = chunks < plan.n_splits ? (int)chunks : plan.n_splits;  // a function of the shapes alone
  double* sums = workspace + (int64_t)plan.n_splits * plan.n_jobs * kTile * kTile;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)plan.n_jobs, (unsigned)n_splits);
  const bool vec = F % 4 == 0 && ((uintptr_t)X & 15) == 0;
  auto tile = weighted ? (vec ? moments_tile_kernel<true, true> : moments_tile_kernel<false, true>)
                       : (vec ? moments_tile_kernel<true, false> : moments_tile_kernel<false, false>);
  hipLaunchKernelGGL(tile, grid, dim3(kMomThreads), 0, s, X, weights, T, F, (int)lag, P, n_pairs, n_splits, plan.nt, plan.n_tri,
                     plan.n_jobs, workspace);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(weighted ? moments_sums_kernel<true> : moments_sums_kernel<false>, dim3((unsigned)((F + 63) / 64), (unsigned)n_splits),
                     dim3(kMomThreads), 0, s, X, weights, T, F, (int)lag, P, n_pairs, n_splits, sums);
  TW_LAUNCH_CHECK();
  const int64_t entries = 2 * (int64_t)F + 3 * (int64_t)F * F;
  hipLaunchKernelGGL(moments_reduce_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, s, workspace, sums, F, n_splits,
                     plan.nt, plan.n_tri, plan.n_jobs, acc, n_pairs_out, (int64_t)n_pairs);
  TW_LAUNCH_CHECK();
  if (weighted && sum_w_out) {
    // the tiles' partials have been read: the head of the workspace (at least one tile, 16384 doubles) holds the ranges' sums
    const int64_t want = ((int64_t)n_pairs + kWsumThreads - 1) / kWsumThreads;
    const int nb = want < kWsumMaxBlocks ? (int)want : kWsumMaxBlocks;
    hipLaunchKernelGGL(weights_partial_kernel, dim3((unsigned)nb), dim3(kWsumThreads), 0, s, weights, T, P, n_pairs, workspace);
    TW_LAUNCH_CHECK();
    hipLaunchKernelGGL(weights_total_kernel, dim3(1), dim3(kWsumThreads), 0, s, workspace, nb, sum_w_out);
    TW_LAUNCH_CHECK();
  }
  return TW_OK;
}

}  // namespace

int tw_lagged_moments(const float* X, int64_t n_chains, int64_t n_frames, int32_t n_features, int64_t lag, double* acc,
                      int64_t* n_pairs_out, double* workspace, void* stream) {
  return lagged_moments_launch(X, nullptr, false, n_chains, n_frames, n_features, lag, acc, n_pairs_out, nullptr, workspace, stream);
}

int tw_lagged_moments_weighted(const float* X, const double* weights, int64_t n_chains, int64_t n_frames, int32_t n_features, int64_t lag,
                               double* acc, int64_t* n_pairs_out, double* sum_w_out, double* workspace, void* stream) {
  return lagged_moments_launch(X, weights, true, n_chains, n_frames, n_features, lag, acc, n_pairs_out, sum_w_out, workspace, stream);
}

int tw_project(const float* X, const double* mean, const double* P, const double* offset, double* out, int64_t n_rows, int32_t n_features,
               int32_t k, void* stream) {
  TW_REQUIRE(n_features >= 1 && n_features <= TW_MOMENTS_MAX_FEATURES, "tw_project: n_features %d: 1 .. %d", n_features,
             TW_MOMENTS_MAX_FEATURES);
  TW_REQUIRE(k >= 1 && k <= kProjMaxK, "tw_project: k %d: 1 .. %d", k, kProjMaxK);
  TW_REQUIRE(n_rows >= 0, "tw_project: n_rows %lld", (long long)n_rows);
  if (n_rows == 0) return TW_OK;  // nothing to compute: no launch
  TW_REQUIRE(X && P && out, "NULL pointer argument");
  const int64_t blocks = (n_rows + kProjRows - 1) / kProjRows;
  TW_REQUIRE(blocks <= 0x7fffffffll, "n_rows %lld: too many row blocks", (long long)n_rows);
  const int kc = (k + kProjThreads / kProjRows - 1) / (kProjThreads / kProjRows);
  hipLaunchKernelGGL(project_kernel, dim3((unsigned)blocks), dim3(kProjThreads), project_lds_bytes(k), (hipStream_t)stream, X, mean, P,
                     offset, out, n_rows, (int)n_features, (int)k, kc);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
