// The E(3)-equivariant NVP flow (model_type equivariant_nvp, tw_flow_desc.variant 3): the coupling nets of
// modules/layers/dense_equivariant_coupling_layer.py + feature_processor.py + equivariant_features_basis.py as exact-fp32
// HIP kernels for gfx950.  TW_PATH_SIMPLE only.
//
// One module (scale or shift) of one coupling layer is four kinds of launch:
//   eq_point_kernel      pointwise features p_v = [emb(atom), (|z_v|,) |x_v|]                                   [M, P]
//   eq_rows_kernel       an MLP over atom rows, hidden layers on chip: the two per-atom halves of the pair MLP's first layer
//                        (A_i = W_i p_i + b, B_j = W_j p_j: the first-layer factorisation), the processor's pointwise MLP, psi, gamma
//   eq_pair_kernel       THE hot kernel: one workgroup owns (row, up to 16 query atoms i) x all keys j, walks the pairs in tiles
//                        of 32, builds silu(A_i + B_j + W_r r_ij) from coordinates on the fly, runs the remaining layers of the
//                        processor's relative MLP and the whole following relative MLP (phi) with every activation in LDS on
//                        the fp32 matrix pipe (v_mfma_f32_32x32x2_f32), skips masked keys and reduces over j in the epilogue:
//                        the mean processed feature per atom [M, E] and the mean of phi (scale: [M, E]; shift: weighted by the
//                        relative basis vectors, [M, 3 n_rel_basis]).  Nothing of size V x V reaches memory.
//   eq_finish_kernel     _calc_shift's / the scale's last line -> [M, 3] in the layout the affine-coupling kernel reads
// Reductions are sequential in pair order per (query, channel): no atomics, run-to-run identical.
#include "tw_common.h"

namespace tw {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16 __attribute__((ext_vector_type(16)));

constexpr int EQ_TM = 32;        // rows (pairs or atoms) per tile: one 32-row MFMA tile
constexpr int EQ_LD = 260;       // LDS row stride in floats (260 % 32 == 4: the b128 A-fragment reads of 8 rows cover all banks)
constexpr int EQ_MAXW = 256;     // widest layer
constexpr int EQ_MAXE = 64;      // widest embedding / processed feature
constexpr int EQ_QI = 16;        // query atoms per workgroup of the pair kernel
constexpr int EQ_MAXL = 4;       // linear layers per MLP (3 hidden layers)

struct EqMlp {   // a Linear / SiLU stack: layer l is W[l] [N[l], K[l]] with row stride ldw[l], bias b[l] (may be NULL)
  const float* W[EQ_MAXL];
  const float* b[EQ_MAXL];
  int K[EQ_MAXL], N[EQ_MAXL], ldw[EQ_MAXL];
  int n;
};

__device__ __forceinline__ float eq_silu(float v) { return v / (1.f + expf(-v)); }
__host__ __device__ inline int eq_up8(int k) { return (k + 7) & ~7; }

// out[r][n] = act(sum_k in[r][k] W[n][k] + b[n]) for the 32 rows of a tile, all 256 threads (4 waves; a wave owns output column
// tiles wave, wave + 4, ...).  `in` holds zeros in columns K .. up8(K); `out` gets zeros in columns N .. the end of its last
// 32-column tile.  MFMA 32x32x2: lane l feeds A[row l % 32][k], B[k][col l % 32] with k = l / 32; here a lane reads FOUR
// consecutive k (one b128 from LDS, one from the weight row) and the four MFMAs of a chunk of 8 take k in the order
// (0, 4), (1, 5), (2, 6), (3, 7) - the same permutation on both operands, so the sum is the plain dot product.
// No barrier inside: the caller synchronises before (input complete) and after (output complete).
__device__ __forceinline__ void eq_layer(const float* in, float* out, const float* __restrict__ W, int ldw,
                                         const float* __restrict__ bias, int K, int N, bool act) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = lane & 31, half = lane >> 5;
  const int n_tiles = (N + 31) / 32;
  const int chunks = eq_up8(K) / 8;
  const bool fast = (K % 8 == 0) && (ldw % 4 == 0) && ((reinterpret_cast<uintptr_t>(W) & 15) == 0);
  const float* arow = in + col * EQ_LD + half * 4;
  for (int t0 = wave; t0 < n_tiles; t0 += 8) {
    const int n0 = t0 * 32 + col, n1 = (t0 + 4) * 32 + col;
    const bool two = t0 + 4 < n_tiles;
    const bool ok0 = n0 < N, ok1 = two && n1 < N;
    const float* w0 = W + (int64_t)(ok0 ? n0 : 0) * ldw + half * 4;
    const float* w1 = W + (int64_t)(ok1 ? n1 : 0) * ldw + half * 4;
    f16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    if (fast) {
      const f4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
      for (int kc = 0; kc < chunks; ++kc) {
        const f4 a = *(const f4*)(arow + kc * 8);
        const f4 b0 = ok0 ? *(const f4*)(w0 + kc * 8) : zero;
        const f4 b1 = ok1 ? *(const f4*)(w1 + kc * 8) : zero;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0[t], acc0, 0, 0, 0);
          if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1[t], acc1, 0, 0, 0);
        }
      }
    } else {
      for (int kc = 0; kc < chunks; ++kc) {
        const f4 a = *(const f4*)(arow + kc * 8);
        f4 b0, b1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int k = kc * 8 + half * 4 + t;
          b0[t] = (ok0 && k < K) ? w0[kc * 8 + t] : 0.f;
          b1[t] = (ok1 && k < K) ? w1[kc * 8 + t] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0[t], acc0, 0, 0, 0);
          if (two) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1[t], acc1, 0, 0, 0);
        }
      }
    }
    // D layout: element r of lane l is row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32
    const float bias0 = (ok0 && bias) ? bias[n0] : 0.f;
    const float bias1 = (ok1 && bias) ? bias[n1] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 8 * (r >> 2) + 4 * half + (r & 3);
      float v = acc0[r] + bias0;
      if (act) v = eq_silu(v);
      out[row * EQ_LD + n0] = ok0 ? v : 0.f;
      if (two) {
        float u = acc1[r] + bias1;
        if (act) u = eq_silu(u);
        out[row * EQ_LD + n1] = ok1 ? u : 0.f;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// pointwise features (equivariant_features_basis.py:81-88, 144-147): positions coupling [emb, |z_v|, |x_v|], velocities [emb, |x_v|]
// ---------------------------------------------------------------------------------------------------------------------
__global__ void eq_point_kernel(const float* __restrict__ emb, const int32_t* __restrict__ atom_types,
                                const float* __restrict__ x_velocs, const float* __restrict__ z_other, int64_t n_cond, int V,
                                int E, int positions, float* __restrict__ pf, int64_t M) {
  const int P = E + (positions ? 2 : 1);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= M * P) return;
  const int64_t m = idx / P;
  const int k = (int)(idx % P);
  const int64_t n = m / V;
  const int v = (int)(m % V);
  const int64_t cv = (n % n_cond) * V + v;
  float val;
  if (k < E) {
    val = emb[(int64_t)atom_types[cv] * E + k];
  } else {
    const float* p = (positions && k == E) ? z_other + m * 3 : x_velocs + cv * 3;
    val = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  }
  pf[idx] = val;
}

// ---------------------------------------------------------------------------------------------------------------------
// an MLP over atom rows: x = [X1 | X2] (mode 0) or X1 + X2 (mode 1, K2 == K1) -> layers on chip -> Y [M, N_last]
// ---------------------------------------------------------------------------------------------------------------------
struct EqRowsArgs {
  const float* X1;
  const float* X2;
  int K1, K2, mode;
  EqMlp m;
  float* Y;
  int64_t M;
};

__global__ void __launch_bounds__(256) eq_rows_kernel(EqRowsArgs p) {
  extern __shared__ float eq_lds[];
  float* cur = eq_lds;
  float* nxt = eq_lds + EQ_TM * EQ_LD;
  const int64_t m0 = (int64_t)blockIdx.x * EQ_TM;
  const int K = p.mode == 0 ? p.K1 + p.K2 : p.K1;
  const int K8 = eq_up8(K);
  for (int idx = threadIdx.x; idx < EQ_TM * K8; idx += 256) {
    const int r = idx / K8, k = idx % K8;
    const int64_t m = m0 + r;
    float v = 0.f;
    if (m < p.M && k < K) {
      if (p.mode == 0) v = k < p.K1 ? p.X1[m * p.K1 + k] : p.X2[m * p.K2 + (k - p.K1)];
      else v = p.X1[m * p.K1 + k] + p.X2[m * p.K1 + k];
    }
    cur[r * EQ_LD + k] = v;
  }
  for (int l = 0; l < p.m.n; ++l) {
    __syncthreads();
    eq_layer(cur, nxt, p.m.W[l], p.m.ldw[l], p.m.b[l], p.m.K[l], p.m.N[l], l + 1 < p.m.n);
    float* t = cur; cur = nxt; nxt = t;
  }
  __syncthreads();
  const int N = p.m.N[p.m.n - 1];
  for (int idx = threadIdx.x; idx < EQ_TM * N; idx += 256) {
    const int r = idx / N, k = idx % N;
    if (m0 + r < p.M) p.Y[(m0 + r) * N + k] = cur[r * EQ_LD + k];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// the fused pair kernel
// ---------------------------------------------------------------------------------------------------------------------
struct EqPairArgs {
  const float* A;       // [M, Hd]  W_i p_i + b of the processor's relative MLP, first layer
  const float* B;       // [M, Hd]  W_j p_j
  const float* Wr;      // first-layer columns of the relative state features: Wr[k * ldwr + f], f < R
  int ldwr, R;
  EqMlp m1;             // the remaining layers of feature_processor._relative_features_mlp (-> E)
  EqMlp m2;             // _shift_with_relative_mlp (-> n_rel_basis) / _scale_with_relative_mlp (-> E)
  const float* x;       // [n_cond, V, 3] centred conditioning coordinates
  const float* z;       // [n_rows, V, 3] the untransformed latent (velocities coupling: z coordinates), else unused
  const uint8_t* masked;  // [n_cond, V]
  int64_t n_cond;
  int V, Hd, E, positions, shift, NR;
  float* avg;           // [M, E]   (1/n) sum_{j unmasked} processed relative feature
  float* rel;           // [M, NR]  scale: (1/n) sum_j phi(h_ij), NR = E; shift: (1/n) sum_j phi_b(h_ij) e_ij^b, NR = 3 n_rel_basis
};

__global__ void __launch_bounds__(256) eq_pair_kernel(EqPairArgs p) {
  extern __shared__ float eq_lds[];
  float* cur = eq_lds;
  float* nxt = eq_lds + EQ_TM * EQ_LD;
  float* accG = eq_lds + 2 * EQ_TM * EQ_LD;        // [EQ_QI][EQ_MAXE]
  float* accR = accG + EQ_QI * EQ_MAXE;            // [EQ_QI][EQ_MAXE]
  float* rdx = accR + EQ_QI * EQ_MAXE;             // [32][3]  x_i - x_j
  float* rdz = rdx + EQ_TM * 3;                    // [32][3]  z_i - z_j
  float* rft = rdz + EQ_TM * 3;                    // [32][2]  relative state features
  int* rqi = (int*)(rft + EQ_TM * 2);              // [32] query index within the block
  int* rj = rqi + EQ_TM;                           // [32] key atom
  int* rok = rj + EQ_TM;                           // [32] pair exists and its key is unmasked
  __shared__ int n_unmasked;

  const int V = p.V, Hd = p.Hd, E = p.E;
  const int qblocks = (V + EQ_QI - 1) / EQ_QI;
  const int64_t n = blockIdx.x / qblocks;
  const int q0 = (int)(blockIdx.x % qblocks) * EQ_QI;
  const int nq = min(EQ_QI, V - q0);
  const int64_t c = n % p.n_cond;
  const uint8_t* mk = p.masked + c * V;
  const float* xs = p.x + c * V * 3;
  const float* zs = p.z + n * (int64_t)V * 3;
  const int tid = threadIdx.x;

  for (int i = tid; i < 2 * EQ_QI * EQ_MAXE; i += 256) accG[i] = 0.f;
  if (tid < 64) {   // atoms of this molecule (wave 0)
    int cnt = 0;
    for (int j = tid; j < V; j += 64) cnt += mk[j] ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (tid == 0) n_unmasked = cnt;
  }
  const int npairs = nq * V;
  const int Hd8 = eq_up8(Hd);
  for (int p0 = 0; p0 < npairs; p0 += EQ_TM) {
    __syncthreads();   // the previous tile's reductions are done with the row table and the buffers
    if (tid < EQ_TM) {
      const int pr = p0 + tid;
      const bool valid = pr < npairs;
      const int qi = valid ? pr / V : 0, j = valid ? pr % V : 0;
      const int i = q0 + qi;
      const float dx0 = xs[i * 3] - xs[j * 3], dx1 = xs[i * 3 + 1] - xs[j * 3 + 1], dx2 = xs[i * 3 + 2] - xs[j * 3 + 2];
      const float xn = sqrtf(dx0 * dx0 + dx1 * dx1 + dx2 * dx2);
      rdx[tid * 3] = dx0; rdx[tid * 3 + 1] = dx1; rdx[tid * 3 + 2] = dx2;
      if (p.positions) {
        rft[tid * 2] = xn;      // |x_i - x_j|
        rft[tid * 2 + 1] = 0.f;
      } else {
        const float dz0 = zs[i * 3] - zs[j * 3], dz1 = zs[i * 3 + 1] - zs[j * 3 + 1], dz2 = zs[i * 3 + 2] - zs[j * 3 + 2];
        rdz[tid * 3] = dz0; rdz[tid * 3 + 1] = dz1; rdz[tid * 3 + 2] = dz2;
        rft[tid * 2] = sqrtf(dz0 * dz0 + dz1 * dz1 + dz2 * dz2);   // (|z_i - z_j|, |x_i - x_j|)
        rft[tid * 2 + 1] = xn;
      }
      rqi[tid] = qi;
      rj[tid] = j;
      rok[tid] = (valid && !mk[j]) ? 1 : 0;
    }
    __syncthreads();
    // first layer, factorised: silu(A_i + B_j + W_r r_ij)
    for (int idx = tid; idx < EQ_TM * Hd8; idx += 256) {
      const int r = idx / Hd8, k = idx % Hd8;
      float v = 0.f;
      if (k < Hd) {
        const int64_t mi = n * V + q0 + rqi[r], mj = n * V + rj[r];
        v = p.A[mi * Hd + k] + p.B[mj * Hd + k] + p.Wr[(int64_t)k * p.ldwr] * rft[r * 2];
        if (p.R == 2) v += p.Wr[(int64_t)k * p.ldwr + 1] * rft[r * 2 + 1];
        v = eq_silu(v);
      }
      cur[r * EQ_LD + k] = v;
    }
    for (int l = 0; l < p.m1.n; ++l) {
      __syncthreads();
      eq_layer(cur, nxt, p.m1.W[l], p.m1.ldw[l], p.m1.b[l], p.m1.K[l], p.m1.N[l], l + 1 < p.m1.n);
      float* t = cur; cur = nxt; nxt = t;
    }
    __syncthreads();
    // the processed relative features of this tile: their masked sum over j (feature_processor.py:60-71) ...
    if (tid < E) {
      for (int r = 0; r < EQ_TM; ++r)
        if (rok[r]) accG[rqi[r] * EQ_MAXE + tid] += cur[r * EQ_LD + tid];
    }
    // ... and through phi; nxt was last read before the barrier above
    for (int l = 0; l < p.m2.n; ++l) {
      if (l > 0) __syncthreads();
      eq_layer(cur, nxt, p.m2.W[l], p.m2.ldw[l], p.m2.b[l], p.m2.K[l], p.m2.N[l], l + 1 < p.m2.n);
      float* t = cur; cur = nxt; nxt = t;
    }
    __syncthreads();
    if (tid < p.NR) {
      if (p.shift) {   // coefficient b times its relative basis vector (positions: x_i - x_j; velocities: z_i - z_j, x_i - x_j)
        const int b = tid / 3, dd = tid % 3;
        const float* e = (p.positions || b == 1) ? rdx : rdz;
        for (int r = 0; r < EQ_TM; ++r)
          if (rok[r]) accR[rqi[r] * EQ_MAXE + tid] += cur[r * EQ_LD + b] * e[r * 3 + dd];
      } else {
        for (int r = 0; r < EQ_TM; ++r)
          if (rok[r]) accR[rqi[r] * EQ_MAXE + tid] += cur[r * EQ_LD + tid];
      }
    }
  }
  __syncthreads();
  const float nf = (float)n_unmasked;
  for (int idx = tid; idx < nq * E; idx += 256) {
    const int qi = idx / E, k = idx % E;
    p.avg[(n * V + q0 + qi) * E + k] = accG[qi * EQ_MAXE + k] / nf;
  }
  for (int idx = tid; idx < nq * p.NR; idx += 256) {
    const int qi = idx / p.NR, k = idx % p.NR;
    p.rel[(n * V + q0 + qi) * p.NR + k] = accR[qi * EQ_MAXE + k] / nf;
  }
}

constexpr int EQ_ROWS_LDS = 2 * EQ_TM * EQ_LD * 4;
constexpr int EQ_PAIR_LDS = EQ_ROWS_LDS + (2 * EQ_QI * EQ_MAXE + EQ_TM * 8 + EQ_TM * 3) * 4;

// ---------------------------------------------------------------------------------------------------------------------
// the module's last line -> out [M, 3]
//   scale (dense_equivariant_coupling_layer.py:375-400): log s_i, one value per atom, repeated over xyz
//   shift (_calc_shift, :150-194): all_shifts = pointwise_shift [.., n_pw, 3] + relative_shift [.., n_rel, 3] BROADCAST (n_pw, n_rel
//   are (2, 1) or (1, 2)), summed over the basis axis, / n:  positions (pw0 + pw1 + 2 rel0) / n, velocities (2 pw0 + rel0 + rel1) / n
// ---------------------------------------------------------------------------------------------------------------------
__global__ void eq_finish_kernel(const float* __restrict__ psi, const float* __restrict__ rel, const float* __restrict__ x_velocs,
                                 const float* __restrict__ z_other, const uint8_t* __restrict__ masked, int64_t n_cond, int V,
                                 int positions, int shift, float* __restrict__ out, int64_t M) {
  const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  if (!shift) {
    const float ls = psi[m];
    out[m * 3] = ls; out[m * 3 + 1] = ls; out[m * 3 + 2] = ls;
    return;
  }
  const int64_t n = m / V;
  const int v = (int)(m % V);
  const int64_t c = n % n_cond;
  int cnt = 0;
  for (int j = 0; j < V; ++j) cnt += masked[c * V + j] ? 0 : 1;
  const float nf = (float)cnt;
  const float* xv = x_velocs + (c * V + v) * 3;
  for (int dd = 0; dd < 3; ++dd) {
    float s;
    if (positions) {
      const float pw0 = psi[m * 2] * z_other[m * 3 + dd], pw1 = psi[m * 2 + 1] * xv[dd];
      const float r0 = rel[m * 3 + dd];
      s = (pw0 + r0) + (pw1 + r0);
    } else {
      const float pw0 = psi[m] * xv[dd];
      s = (pw0 + rel[m * 6 + dd]) + (pw0 + rel[m * 6 + 3 + dd]);
    }
    out[m * 3 + dd] = s / nf;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// raw layout (mirrored by timewarp_amd/weights.py): every tensor with at least one axis starts at a multiple of 4 floats
// ---------------------------------------------------------------------------------------------------------------------
inline int64_t al4(int64_t o) { return (o + 3) & ~(int64_t)3; }

struct EqMlpOff {
  int64_t w[EQ_MAXL], b[EQ_MAXL];
  int K[EQ_MAXL], N[EQ_MAXL];
  int n;
};
struct EqModuleOff {
  EqMlpOff rel_feat, pw_feat, with_pw, with_rel, gamma;
};

int64_t eq_mlp_off(const tw_flow_desc& d, int in, int out, int64_t o, EqMlpOff* m) {
  m->n = d.n_hidden + 1;
  for (int l = 0; l < m->n; ++l) {
    m->K[l] = l == 0 ? in : d.d_hidden;
    m->N[l] = l == d.n_hidden ? out : d.d_hidden;
    o = al4(o); m->w[l] = o; o += (int64_t)m->N[l] * m->K[l];
    o = al4(o); m->b[l] = o; o += m->N[l];
  }
  return o;
}

// offsets of module `net` (0 scale, 1 shift) of a coupling layer; returns the offset behind it
int64_t eq_module_off(const tw_flow_desc& d, bool positions, int net, int64_t o, EqModuleOff* m) {
  const int E = d.d_emb;
  const int P = E + (positions ? 2 : 1), R = positions ? 1 : 2;
  const int n_pw = positions ? 2 : 1, n_rel = positions ? 1 : 2;
  o = eq_mlp_off(d, 2 * P + R, E, o, &m->rel_feat);
  o = eq_mlp_off(d, P + E, E, o, &m->pw_feat);
  o = eq_mlp_off(d, E, net == 0 ? E : n_pw, o, &m->with_pw);
  o = eq_mlp_off(d, E, net == 0 ? E : n_rel, o, &m->with_rel);
  if (net == 0) o = eq_mlp_off(d, E, 1, o, &m->gamma);
  return o;
}

struct EqWs {
  float *pf, *A, *B, *avg, *rel, *pw, *psi, *ls, *out;
  int64_t bytes;
};

EqWs eq_ws(const tw_flow_desc& d, int64_t n_rows, int V, void* base) {
  EqWs w;
  const int64_t M = n_rows * V;
  char* p = (char*)base;
  auto take = [&](int64_t floats) {
    float* r = (float*)p;
    p += (floats * 4 + 255) / 256 * 256;
    return r;
  };
  w.pf = take(M * (d.d_emb + 2));
  w.A = take(M * d.d_hidden);
  w.B = take(M * d.d_hidden);
  w.avg = take(M * d.d_emb);
  w.rel = take(M * (d.d_emb > 6 ? d.d_emb : 6));
  w.pw = take(M * d.d_emb);
  w.psi = take(M * (d.d_emb > 2 ? d.d_emb : 2));
  w.ls = take(M);
  w.out = take(M * 3);
  w.bytes = p - (char*)base;
  return w;
}

EqMlp eq_mlp(const float* raw, const EqMlpOff& o, int first = 0) {
  EqMlp m{};
  m.n = o.n - first;
  for (int l = first; l < o.n; ++l) {
    m.W[l - first] = raw + o.w[l];
    m.b[l - first] = raw + o.b[l];
    m.K[l - first] = o.K[l];
    m.N[l - first] = o.N[l];
    m.ldw[l - first] = o.K[l];
  }
  return m;
}

LdsLimit g_rows_lds, g_pair_lds;

int launch_rows(const float* X1, int K1, const float* X2, int K2, int mode, const EqMlp& m, float* Y, int64_t M, hipStream_t s) {
  int rc;
  if ((rc = g_rows_lds.ensure((const void*)eq_rows_kernel, EQ_ROWS_LDS))) return rc;
  EqRowsArgs p{X1, X2, K1, K2, mode, m, Y, M};
  hipLaunchKernelGGL(eq_rows_kernel, dim3((unsigned)((M + EQ_TM - 1) / EQ_TM)), dim3(256), EQ_ROWS_LDS, s, p);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

// one module of coupling layer c on stream s; out [M, 3]: log-scale repeated over xyz (net 0) or the shift (net 1)
int eq_module(const FlowArgs& a, const EqWs& w, int c, int net, const float* z_other, float* out, hipStream_t s) {
  const tw_flow_desc& d = *a.desc;
  const RawLayout L = raw_layout(d);
  const int V = a.n_atoms, E = d.d_emb, Hd = d.d_hidden;
  const int64_t M = a.n_rows * V;
  const bool positions = (c % 2) == d.pos_mod2;
  const int P = E + (positions ? 2 : 1), R = positions ? 1 : 2;
  const int n_rel = positions ? 1 : 2;
  // walk the layout up to (c, net)
  int64_t o = L.chain;
  EqModuleOff mo;
  for (int cc = 0, done = 0; cc <= c && !done; ++cc)
    for (int nn = 0; nn < 2 && !done; ++nn) {
      o = eq_module_off(d, (cc % 2) == d.pos_mod2, nn, o, &mo);
      done = cc == c && nn == net;
    }
  int rc;
  const int64_t MP = M * P;
  hipLaunchKernelGGL(eq_point_kernel, dim3((unsigned)((MP + 255) / 256)), dim3(256), 0, s, a.raw + L.emb, a.atom_types, a.x_velocs,
                     z_other, a.n_cond, V, E, positions ? 1 : 0, w.pf, M);
  TW_LAUNCH_CHECK();
  // first layer of the processor's relative MLP, per atom: input order [p_i | p_j | r_ij] (feature_processor.py:53-55)
  const int K0 = 2 * P + R;
  EqMlp first{};
  first.n = 1;
  first.W[0] = a.raw + mo.rel_feat.w[0]; first.b[0] = a.raw + mo.rel_feat.b[0];
  first.K[0] = P; first.N[0] = Hd; first.ldw[0] = K0;
  if ((rc = launch_rows(w.pf, P, nullptr, 0, 0, first, w.A, M, s))) return rc;
  first.W[0] = a.raw + mo.rel_feat.w[0] + P; first.b[0] = nullptr;
  if ((rc = launch_rows(w.pf, P, nullptr, 0, 0, first, w.B, M, s))) return rc;
  EqPairArgs pa{};
  pa.A = w.A; pa.B = w.B;
  pa.Wr = a.raw + mo.rel_feat.w[0] + 2 * P; pa.ldwr = K0; pa.R = R;
  pa.m1 = eq_mlp(a.raw, mo.rel_feat, 1);
  pa.m2 = eq_mlp(a.raw, mo.with_rel);
  pa.x = a.x_coords; pa.z = z_other; pa.masked = a.masked; pa.n_cond = a.n_cond;
  pa.V = V; pa.Hd = Hd; pa.E = E; pa.positions = positions ? 1 : 0; pa.shift = net;
  pa.NR = net == 0 ? E : 3 * n_rel;
  pa.avg = w.avg; pa.rel = w.rel;
  if ((rc = g_pair_lds.ensure((const void*)eq_pair_kernel, EQ_PAIR_LDS))) return rc;
  const int64_t blocks = a.n_rows * ((V + EQ_QI - 1) / EQ_QI);
  TW_REQUIRE(blocks < ((int64_t)1 << 31), "equivariant flow: %lld workgroups exceed the grid", (long long)blocks);
  hipLaunchKernelGGL(eq_pair_kernel, dim3((unsigned)blocks), dim3(256), EQ_PAIR_LDS, s, pa);
  TW_LAUNCH_CHECK();
  // processed pointwise features (feature_processor.py:72-77), psi, and for the scale gamma(psi + mean phi)
  if ((rc = launch_rows(w.pf, P, w.avg, E, 0, eq_mlp(a.raw, mo.pw_feat), w.pw, M, s))) return rc;
  if ((rc = launch_rows(w.pw, E, nullptr, 0, 0, eq_mlp(a.raw, mo.with_pw), w.psi, M, s))) return rc;
  const float* last = w.psi;
  if (net == 0) {
    if ((rc = launch_rows(w.psi, E, w.rel, E, 1, eq_mlp(a.raw, mo.gamma), w.ls, M, s))) return rc;
    last = w.ls;
  }
  hipLaunchKernelGGL(eq_finish_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, last, w.rel, a.x_velocs, z_other, a.masked,
                     a.n_cond, V, positions ? 1 : 0, net, out, M);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

}  // namespace

bool equivariant_desc_ok(const tw_flow_desc& d) {
  return d.d_emb <= EQ_MAXE && d.d_hidden <= EQ_MAXW && d.d_hidden % 8 == 0 && d.n_hidden >= 1 && d.n_hidden < EQ_MAXL;
}

void equivariant_raw_layout(const tw_flow_desc& d, RawLayout* L) {
  L->d_in = 0;
  L->emb = 0;
  L->lengthscales = al4((int64_t)d.n_elements * d.d_emb);
  L->prior = L->lengthscales;
  L->chain = L->prior + 2;
  L->rff = L->nets = 0;
  L->coupling_size = 0;   // (couplings alternate between two shapes: walk with eq_module_off)
  int64_t o = L->chain;
  EqModuleOff mo;
  for (int c = 0; c < d.n_coupling; ++c)
    for (int net = 0; net < 2; ++net) o = eq_module_off(d, (c % 2) == d.pos_mod2, net, o, &mo);
  L->total = o;
}

int64_t equivariant_workspace_bytes(const tw_flow_desc& d, int64_t n_rows, int n_atoms) {
  return 2 * eq_ws(d, n_rows, n_atoms, nullptr).bytes;   // one set of buffers per module: the two run on two streams
}

int flow_pass_equivariant(const FlowArgs& a) {
  const tw_flow_desc& d = *a.desc;
  TW_REQUIRE(!a.simple_h3, "equivariant flow: no split-fp16 kernels (TW_PATH_SIMPLE only)");
  const EqWs w = eq_ws(d, a.n_rows, a.n_atoms, a.ws);
  TW_REQUIRE_WORKSPACE(2 * w.bytes, a.ws_bytes);
  const EqWs w2 = eq_ws(d, a.n_rows, a.n_atoms, (char*)a.ws + w.bytes);
  SideFork f;   // (an error return between fork and join brings the side stream back: it writes the second half of the caller's workspace)
  int rc;
  if ((rc = f.init(SIDE_FLOW, a.stream))) return rc;
  for (int i = 0; i < d.n_coupling; ++i) {
    const int c = a.reverse ? d.n_coupling - 1 - i : i;
    const bool positions = (c % 2) == d.pos_mod2;
    const float* z_other = positions ? a.z_velocs : a.z_coords;
    float* z_t = positions ? a.z_coords : a.z_velocs;
    if ((rc = f.fork())) return rc;
    if ((rc = eq_module(a, w2, c, 1, z_other, w2.out, f.side))) return rc;
    if ((rc = eq_module(a, w, c, 0, z_other, w.out, a.stream))) return rc;
    if ((rc = f.join())) return rc;
    if ((rc = launch_coupling(w.out, w2.out, a.masked, a.n_cond, z_t, a.delta_logp, a.n_rows, a.n_atoms, a.reverse, a.stream,
                              nullptr, a.desc->range_flag)))
      return rc;
  }
  return TW_OK;
}

int debug_module_equivariant(const FlowArgs& a, int c, int net, const float* z_other, float* dump) {
  const tw_flow_desc& d = *a.desc;
  const EqWs w = eq_ws(d, a.n_rows, a.n_atoms, a.ws);
  TW_REQUIRE_WORKSPACE(w.bytes, a.ws_bytes);
  return eq_module(a, w, c, net, z_other, dump, a.stream);
}

}  // namespace tw
