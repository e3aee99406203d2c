// Weight-stream packing: the one executor behind every packed stream (tw_flow_pack, _h3, _h1, _simple_h3).
//
// The layout walks (pack_weights / dense_pack_weights / h3_pack_weights) only append ops to a PackPlan; PackPlan::run
// uploads the table, zeroes the destination and runs two launches: the absmax of every scale group (each into its own
// slot), then every op's work items (one wave each), found through the prefix of the ops' item counts.  This file is the
// one place that knows the element order of the three tile formats:
//   PACK_F32  (TILE_F, 1 KiB)       tile (ot, ft) element (lane, r) = W[row0 + 16 ot + (lane&15)][col0 + 16 ft + 4 (lane>>4) + r]
//   PACK_PAIR (H3_PAIR_BYTES, 2 KiB) tile (ot, ks) element (lane, e) = W[row0 + 16 ot + (lane&15)][col0 + 32 ks + 16 (e/4) + 4 (lane>>4) + e%4]
//                                    as fp16 hi at byte 16 lane + 2 e and fp16 lo = fp16(v - hi) 1 KiB further
//   PACK_HI   (1 KiB)               the same element order, fp16 hi only
// tiles ordered ot-major over (n_ot, n_ks); rows / columns outside (rows_valid, cols_valid) are zero.
#include "tw_common.h"

namespace tw {

#define H3_TARGET_MAX 4096.0f  // |w| * 2^s is scaled up to just below this

// folded attention weight of head h: Wc[o][i] = sum_k Wo[o][h*128+k] * Wv[h*128+k][i], fp64 accumulate
__device__ __forceinline__ double fold_elem(const float* wv, const float* wo, int H, int h, int o_row, int i_col) {
  double acc = 0.0;
  for (int k = 0; k < 128; ++k)
    acc += (double)wo[(int64_t)o_row * (H * 128) + h * 128 + k] * (double)wv[(int64_t)(h * 128 + k) * 128 + i_col];
  return acc;
}

// scale exponent: largest power of two with max * 2^s < H3_TARGET_MAX (0 for an all-zero or non-finite group)
__device__ int scale_exp(float m) {
  int s = 0;
  if (m > 0.f && isfinite(m)) {
    s = (int)floorf(log2f(H3_TARGET_MAX / m));
    if (s > 24) s = 24;
    if (s < -24) s = -24;
    while (ldexpf(m, s) >= H3_TARGET_MAX) --s;
  }
  return s;
}

// grid (64, groups) x 256: fmaxf ignores NaN and the atomic max of non-negative float bits is order independent, so the
// slot's bits do not depend on the grid
__global__ void __launch_bounds__(256) pack_absmax_kernel(const PackGroup* __restrict__ groups, float* __restrict__ absmax) {
  const PackGroup G = groups[blockIdx.y];
  const int64_t n = G.wo ? (int64_t)G.n * 128 * 128 : G.n;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(i % (128 * 128));
    m = fmaxf(m, fabsf(G.wo ? (float)fold_elem(G.src, G.wo, (int)G.n, (int)(i / (128 * 128)), e / 128, e % 128) : G.src[i]));
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax((int*)(absmax + blockIdx.y), __float_as_int(m));  // m >= 0: int order = float order
}

// one wave per work item: item i belongs to the last op with first[op] <= i
__global__ void __launch_bounds__(256) pack_ops_kernel(const PackOp* __restrict__ ops, const int64_t* __restrict__ first,
                                                      int n_ops, const float* __restrict__ absmax) {
  const int64_t item = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (item >= first[n_ops]) return;
  int lo = 0, up = n_ops - 1;
  while (lo < up) {
    const int mid = (lo + up + 1) >> 1;
    if (first[mid] <= item) lo = mid;
    else up = mid - 1;
  }
  const PackOp& op = ops[lo];
  const int64_t t = item - first[lo];
  const int s = op.group >= 0 ? scale_exp(absmax[op.group]) : 0;
  if (op.kind == PACK_COPY) {
    const int64_t i = t * 64 + lane;
    if (i < op.n_pad) ((float*)op.dst)[i] = i < op.n ? op.src[i] : 0.f;
    return;
  }
  if (op.kind == PACK_SCALAR) {
    if (lane == 0) *(float*)op.dst = ldexpf(1.f, -s);
    return;
  }
  const float sc = ldexpf(1.f, s);
  const int ot = (int)(t / op.n_ks), ks = (int)(t % op.n_ks);
  const int row = op.row0 + 16 * ot + (lane & 15);
  // element value (unscaled in the f32 format) and, in the fp16 formats, its hi half: a folded element's hi is rounded from
  // the fp64 product in one step, as the compiled per-tile kernels did (their fp64 -> fp32 -> fp16 chain folded into one)
  auto elem = [&](int col, _Float16& hi) -> float {
    if (op.kind == PACK_FOLD) {
      const double acc = fold_elem(op.src, op.wo, op.H, op.h, row, col);
      if (op.fmt == PACK_F32) return (float)acc;
      hi = (_Float16)(acc * (double)sc);
      return (float)(acc * (double)sc);
    }
    const float x = row < op.rows_valid && col < op.cols_valid ? op.src[(int64_t)row * op.ld + col] : 0.f;
    hi = (_Float16)(x * sc);
    return op.fmt == PACK_F32 ? x : x * sc;
  };
  _Float16 hi;
  if (op.fmt == PACK_F32) {
    float* o = (float*)op.dst + (t * 64 + lane) * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = elem(op.col0 + 16 * ks + 4 * (lane >> 4) + r, hi);
    return;
  }
  char* tile = (char*)op.dst + t * (op.fmt == PACK_HI ? 1024 : 2048);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float v = elem(op.col0 + 32 * ks + 16 * (e / 4) + 4 * (lane >> 4) + (e % 4), hi);
    ((_Float16*)(tile + lane * 16))[e] = hi;
    if (op.fmt == PACK_PAIR) ((_Float16*)(tile + 1024 + lane * 16))[e] = (_Float16)(v - (float)hi);
  }
}

int PackPlan::run(void* dst, int64_t dst_bytes, hipStream_t s) const {
  TW_HIP_CHECK(hipMemsetAsync(dst, 0, dst_bytes, s));
  const int n_ops = (int)ops.size(), n_groups = (int)groups.size();
  TW_REQUIRE(n_groups < 65536, "pack: %d scale groups", n_groups);
  std::vector<int64_t> first(n_ops + 1, 0);  // first work item of every op, then the total
  for (int i = 0; i < n_ops; ++i) {
    const PackOp& op = ops[i];
    first[i + 1] = first[i] + (op.kind == PACK_COPY ? (op.n_pad + 63) / 64 : op.kind == PACK_SCALAR ? 1 : (int64_t)op.n_ot * op.n_ks);
  }
  const int64_t blocks = (first[n_ops] + 3) / 4;
  TW_REQUIRE(blocks < (int64_t)1 << 31, "pack: %lld work items", (long long)first[n_ops]);
  if (n_ops == 0) return TW_OK;
  // one temporary allocation: [absmax slots, zero][first][groups][ops]
  const size_t o_first = ((size_t)n_groups * 4 + 15) / 16 * 16, o_groups = o_first + first.size() * 8,
               o_ops = o_groups + groups.size() * sizeof(PackGroup), bytes = o_ops + ops.size() * sizeof(PackOp);
  std::vector<char> host(bytes, 0);
  memcpy(host.data() + o_first, first.data(), first.size() * 8);
  if (n_groups) memcpy(host.data() + o_groups, groups.data(), groups.size() * sizeof(PackGroup));
  memcpy(host.data() + o_ops, ops.data(), ops.size() * sizeof(PackOp));
  char* tmp = nullptr;
  TW_HIP_CHECK(hipMalloc(&tmp, bytes));
  auto launch = [&]() -> int {
    TW_HIP_CHECK(hipMemcpyAsync(tmp, host.data(), bytes, hipMemcpyHostToDevice, s));
    if (n_groups) {
      hipLaunchKernelGGL(pack_absmax_kernel, dim3(64, n_groups), dim3(256), 0, s, (const PackGroup*)(tmp + o_groups), (float*)tmp);
      TW_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pack_ops_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const PackOp*)(tmp + o_ops),
                       (const int64_t*)(tmp + o_first), n_ops, (const float*)tmp);
    TW_LAUNCH_CHECK();
    return TW_OK;
  };
  const int rc = launch();
  const hipError_t e = hipStreamSynchronize(s);  // the table and the slots must outlive the launches
  const hipError_t f = hipFree(tmp);
  if (rc) return rc;
  TW_HIP_CHECK(e);
  TW_HIP_CHECK(f);
  return TW_OK;
}

}  // namespace tw
