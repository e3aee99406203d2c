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

// ---- cloud coverage --------------------------------------------------------------------------------------------------------------
// min over a group's cloud points of the squared distance to every reference point, then the largest of those minima per group: the
// all-pairs pass of the speed-up notebooks without the M x N matrix.  A workgroup owns kCovRefBlock reference points (kCovRefPerLane per
// lane, in registers, with their running minima), one group and one contiguous range of that group's tiles.  A tile is kCovTile cloud
// points staged through LDS as [point][k]; every lane of a wave reads the same point at the same address (a broadcast, no bank
// conflict), so one LDS read feeds kCovRefPerLane * (2 DIM + 1) fp64 VALU instructions per lane.  The next tile's global loads are issued
// into registers before the current tile is compared.  min and max are exact, so the split of the cloud axis (a function of the shapes
// alone) changes no bit: the ranges' minima go to the workspace, coverage_min_kernel takes their minimum per reference point and the
// largest minimum of each chunk of reference points, coverage_worst_kernel the largest over the chunks.  Ties go to the smallest index
// at every stage.  Nothing is atomic.
constexpr int kCovThreads = 256;
constexpr int kCovRefPerLane = 2;
constexpr int kCovRefBlock = kCovThreads * kCovRefPerLane;  // 512 reference points per workgroup
constexpr int kCovTile = 256;                               // cloud points per tile: DIM * 2 KiB of LDS
constexpr int kCovMinTilesPerSplit = 2;                     // a range of the cloud axis is never shorter than this (but for the last)
constexpr int kCovMaxSplits = 64;
constexpr int kCovTargetBlocks = 2048;                      // 8 workgroups of 4 waves on each of 256 CUs
constexpr int kCovRedPerThread = 8;
constexpr int kCovRedChunk = kCovThreads * kCovRedPerThread;  // reference points per workgroup of coverage_min_kernel
constexpr int64_t kCovMaxBlocks = 1ll << 22;                  // blocks x 256 threads stays below 2^32
static_assert(kCovTile == kCovThreads, "a thread stages entry tid + 256 i of a tile, i < DIM");

struct CoveragePlan {
  int64_t n_rblocks;        // blocks of reference points
  int64_t n_chunks;         // chunks of reference points in the reduction
  int64_t tiles_per_split;  // tiles of one group one workgroup walks
  int n_splits;             // ranges of the cloud axis
  int64_t blocks;           // workgroups of coverage_tile_kernel
};

CoveragePlan coverage_plan(int64_t n_ref, int64_t n_cloud, int64_t n_groups) {
  CoveragePlan p;
  p.n_rblocks = (n_ref + kCovRefBlock - 1) / kCovRefBlock;
  p.n_chunks = (n_ref + kCovRedChunk - 1) / kCovRedChunk;
  const int64_t per_group = (n_cloud + n_groups - 1) / n_groups;  // the largest group
  const int64_t nt = (per_group + kCovTile - 1) / kCovTile;
  const int64_t base = p.n_rblocks * n_groups;
  int64_t want = (kCovTargetBlocks + base - 1) / base;
  const int64_t by_tiles = nt / kCovMinTilesPerSplit;
  if (want > by_tiles) want = by_tiles;
  if (want > kCovMaxSplits) want = kCovMaxSplits;
  if (want < 1) want = 1;
  p.tiles_per_split = nt > 0 ? (nt + want - 1) / want : 1;
  p.n_splits = nt > 0 ? (int)((nt + p.tiles_per_split - 1) / p.tiles_per_split) : 1;
  p.blocks = base * p.n_splits;
  return p;
}

// the refusals the size query and the call share; NULL when the shapes are supported
const char* coverage_refusal(int64_t n_ref, int64_t n_cloud, int32_t dim, int32_t n_groups) {
  if (dim < 1 || dim > TW_COVERAGE_MAX_DIM) return "dim: 1 .. 8";
  if (n_ref < 1) return "n_ref: at least 1";
  if (n_cloud < 0) return "n_cloud: at least 0";
  if (n_groups < 1) return "n_groups: at least 1";
  if (n_ref > (1ll << 31) || n_groups > kCovMaxBlocks || n_cloud > (1ll << 40)) return "n_ref <= 2^31, n_groups <= 2^22, n_cloud <= 2^40";
  if (coverage_plan(n_ref, n_cloud, n_groups).blocks > kCovMaxBlocks) return "ceil(n_ref / 512) x n_groups x splits: at most 2^22 workgroups";
  return nullptr;
}

int64_t coverage_workspace_bytes(const CoveragePlan& p, int64_t n_ref, int64_t n_groups) {
  return (int64_t)sizeof(double) * ((int64_t)p.n_splits * n_groups * n_ref + 2 * n_groups * p.n_chunks);
}

template <int DIM>
__global__ __launch_bounds__(kCovThreads) void coverage_tile_kernel(const double* __restrict__ ref, const double* __restrict__ cloud,
                                                                    int64_t n_ref, int64_t n_cloud, int64_t n_groups, int64_t n_rblocks,
                                                                    int64_t tiles_per_split, double* __restrict__ part) {
  __shared__ double Cs[kCovTile * DIM];
  const int tid = threadIdx.x;
  const int64_t rb = (int64_t)blockIdx.x % n_rblocks, rest = (int64_t)blockIdx.x / n_rblocks;
  const int64_t g = rest % n_groups, split = rest / n_groups;
  // group g holds the cloud rows g, g + G, g + 2 G, ...: `cnt` of them, numbered 0 .. cnt - 1 here
  const int64_t cnt = g < n_cloud ? (n_cloud - g + n_groups - 1) / n_groups : 0;
  const int64_t lo = split * tiles_per_split * kCovTile, hi = lo + tiles_per_split * kCovTile;
  const int64_t p_begin = lo < cnt ? lo : cnt, p_end = hi < cnt ? hi : cnt;

  double r[kCovRefPerLane][DIM], m[kCovRefPerLane];
#pragma unroll
  for (int q = 0; q < kCovRefPerLane; ++q) {
    const int64_t a = rb * kCovRefBlock + q * kCovThreads + tid;
    m[q] = INFINITY;
#pragma unroll
    for (int k = 0; k < DIM; ++k) r[q][k] = a < n_ref ? ref[a * DIM + k] : 0.0;
  }

  // entry e = tid + 256 i of a tile is coordinate e % DIM of its point e / DIM: for one group consecutive threads load consecutive doubles
  double nx[DIM];
  auto fetch = [&](int64_t pb) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const int e = tid + kCovThreads * i;
      const int64_t p = pb + e / DIM;
      nx[i] = p < p_end ? cloud[(g + p * n_groups) * DIM + e % DIM] : 0.0;
    }
  };
  if (p_begin < p_end) fetch(p_begin);
  for (int64_t pb = p_begin; pb < p_end; pb += kCovTile) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int i = 0; i < DIM; ++i) Cs[tid + kCovThreads * i] = nx[i];
    __syncthreads();
    if (pb + kCovTile < p_end) fetch(pb + kCovTile);  // in flight while this tile is compared
    const int np = (int)(p_end - pb < kCovTile ? p_end - pb : kCovTile);
#pragma unroll 4
    for (int p = 0; p < np; ++p) {
      double c[DIM];
#pragma unroll
      for (int k = 0; k < DIM; ++k) c[k] = Cs[p * DIM + k];
#pragma unroll
      for (int q = 0; q < kCovRefPerLane; ++q) {
        const double d0 = r[q][0] - c[0];
        double d2 = d0 * d0;
#pragma unroll
        for (int k = 1; k < DIM; ++k) {
          const double d = r[q][k] - c[k];
          d2 = fma(d, d, d2);
        }
        m[q] = fmin(m[q], d2);
      }
    }
  }
  double* dst = part + (split * n_groups + g) * n_ref;
#pragma unroll
  for (int q = 0; q < kCovRefPerLane; ++q) {
    const int64_t a = rb * kCovRefBlock + q * kCovThreads + tid;
    if (a < n_ref) dst[a] = m[q];
  }
}

// (value, index) with the larger value, on equal values the smaller index
__device__ __forceinline__ void coverage_take(double& v, int64_t& i, double v2, int64_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) v = v2, i = i2;
}

__device__ __forceinline__ void coverage_block_max(double& v, int64_t& i, double* rv, int64_t* ri) {
  rv[threadIdx.x] = v, ri[threadIdx.x] = i;
  __syncthreads();
  for (int s = kCovThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      coverage_take(v, i, rv[threadIdx.x + s], ri[threadIdx.x + s]);
      rv[threadIdx.x] = v, ri[threadIdx.x] = i;
    }
    __syncthreads();
  }
}

// workgroup (chunk c, group g): the minimum over the ranges for the reference points of the chunk, stored to out_min when it is given,
// and the chunk's largest minimum with its smallest index.  A squared distance is >= 0, so -1 is below every candidate.
__global__ __launch_bounds__(kCovThreads) void coverage_min_kernel(const double* __restrict__ part, int n_splits, int64_t n_ref,
                                                                   int64_t n_groups, int64_t n_chunks, double* __restrict__ out_min,
                                                                   double* __restrict__ chunk_v, int64_t* __restrict__ chunk_i) {
  __shared__ double rv[kCovThreads];
  __shared__ int64_t ri[kCovThreads];
  const int64_t c = (int64_t)blockIdx.x % n_chunks, g = (int64_t)blockIdx.x / n_chunks;
  double bv = -1.0;
  int64_t bi = INT64_MAX;
#pragma unroll
  for (int k = 0; k < kCovRedPerThread; ++k) {
    const int64_t a = c * kCovRedChunk + k * kCovThreads + threadIdx.x;
    if (a < n_ref) {
      double v = part[g * n_ref + a];
      for (int s = 1; s < n_splits; ++s) v = fmin(v, part[(s * n_groups + g) * n_ref + a]);
      if (out_min) out_min[g * n_ref + a] = v;
      coverage_take(bv, bi, v, a);
    }
  }
  coverage_block_max(bv, bi, rv, ri);
  if (threadIdx.x == 0) chunk_v[g * n_chunks + c] = bv, chunk_i[g * n_chunks + c] = bi;
}

// workgroup g: the largest of the chunks' maxima, its square root and its index
__global__ __launch_bounds__(kCovThreads) void coverage_worst_kernel(const double* __restrict__ chunk_v, const int64_t* __restrict__ chunk_i,
                                                                     int64_t n_chunks, double* __restrict__ out_worst,
                                                                     int64_t* __restrict__ out_arg) {
  __shared__ double rv[kCovThreads];
  __shared__ int64_t ri[kCovThreads];
  const int64_t g = blockIdx.x;
  double bv = -1.0;
  int64_t bi = INT64_MAX;
  for (int64_t c = threadIdx.x; c < n_chunks; c += kCovThreads) coverage_take(bv, bi, chunk_v[g * n_chunks + c], chunk_i[g * n_chunks + c]);
  coverage_block_max(bv, bi, rv, ri);
  if (threadIdx.x == 0) out_worst[g] = sqrt(bv), out_arg[g] = bi;
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

int64_t tw_cloud_coverage_workspace_bytes(int64_t n_ref, int64_t n_cloud, int32_t dim, int32_t n_groups) {
  if (coverage_refusal(n_ref, n_cloud, dim, n_groups)) return -1;
  return coverage_workspace_bytes(coverage_plan(n_ref, n_cloud, n_groups), n_ref, n_groups);
}

int tw_cloud_coverage(const double* ref, const double* cloud, int64_t n_ref, int64_t n_cloud, int32_t dim, int32_t n_groups,
                      double* out_min_d2, double* out_worst, int64_t* out_arg, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* refusal = coverage_refusal(n_ref, n_cloud, dim, n_groups);
  TW_REQUIRE(!refusal, "tw_cloud_coverage: %s (dim %d, n_ref %lld, n_cloud %lld, n_groups %d)", refusal, dim, (long long)n_ref,
             (long long)n_cloud, n_groups);
  TW_REQUIRE(ref && out_worst && out_arg && workspace && (cloud || n_cloud == 0), "tw_cloud_coverage: NULL pointer argument");
  TW_REQUIRE(((uintptr_t)workspace & 7) == 0, "tw_cloud_coverage: workspace must be 8-byte aligned");
  const CoveragePlan plan = coverage_plan(n_ref, n_cloud, n_groups);
  TW_REQUIRE_WORKSPACE(coverage_workspace_bytes(plan, n_ref, n_groups), workspace_bytes);
  double* part = (double*)workspace;
  double* chunk_v = part + (int64_t)plan.n_splits * n_groups * n_ref;
  int64_t* chunk_i = (int64_t*)(chunk_v + (int64_t)n_groups * plan.n_chunks);
  hipStream_t s = (hipStream_t)stream;
  const int64_t G = n_groups;
#define TW_COVERAGE_LAUNCH(D)                                                                                                          \
  case D:                                                                                                                               \
    hipLaunchKernelGGL(coverage_tile_kernel<D>, dim3((unsigned)plan.blocks), dim3(kCovThreads), 0, s, ref, cloud, n_ref, n_cloud, G, \
                       plan.n_rblocks, plan.tiles_per_split, part);                                                                     \
    break;
  switch (dim) {
    TW_COVERAGE_LAUNCH(1)
    TW_COVERAGE_LAUNCH(2)
    TW_COVERAGE_LAUNCH(3)
    TW_COVERAGE_LAUNCH(4)
    TW_COVERAGE_LAUNCH(5)
    TW_COVERAGE_LAUNCH(6)
    TW_COVERAGE_LAUNCH(7)
    TW_COVERAGE_LAUNCH(8)
  }
#undef TW_COVERAGE_LAUNCH
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(coverage_min_kernel, dim3((unsigned)(plan.n_chunks * G)), dim3(kCovThreads), 0, s, part, plan.n_splits, n_ref, G,
                     plan.n_chunks, out_min_d2, chunk_v, chunk_i);
  TW_LAUNCH_CHECK();
  hipLaunchKernelGGL(coverage_worst_kernel, dim3((unsigned)G), dim3(kCovThreads), 0, s, chunk_v, chunk_i, plan.n_chunks, out_worst, out_arg);
  TW_LAUNCH_CHECK();
  return TW_OK;
}
