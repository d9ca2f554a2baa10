// Fused BatchNorm2d (+residual add)(+ReLU) for gfx950 — training fwd/bwd and
// eval fwd, NHWC (channels_last) fast path + generic fallbacks, fp32/bf16
// activations with fp32 statistics.
//
// These ops are HBM-bound on MI355X; the design rules applied here:
//  * 16 B/lane vector access everywhere (8 bf16 / 4 f32 per thread) — hipcc
//    does not auto-vectorize bf16 loads.
//  * all hot-loop index math in uint32 (64-bit div/mod is ~40 VALU cycles and
//    made the first version 10x off roofline); launchers fall back to the
//    generic kernels when a tensor exceeds 2^31 elements.
//  * NHWC reductions: a thread owns the fixed channels of its first vector,
//    (i*V .. i*V+V-1) mod C, accumulating in registers over a grid-stride
//    loop, one LDS atomicAdd per channel at the end. Valid when C | 2048
//    (every ResNet/UNet width) and the grid stride is a multiple of C, which
//    grid_quantum() guarantees.
//  * statistics are accumulated around a per-channel shift (the first pixel's
//    value on the fast path, the mean of the first 32 pixels on the generic
//    one), so the single-pass E[d^2]-E[d]^2 variance does not cancel when
//    |mean| >> std.
//  * fusion: the residual add and ReLU fold into the normalize pass (fwd) and
//    the dgamma/dbeta pass emits the gated upstream gradient (bwd) so the
//    elementwise add/relu/relu' kernels and their whole-tensor round trips
//    disappear.
#include "tfosr_common.h"

typedef unsigned int u32;

// ---------------------------------------------------------------------------
// load/store helpers: VEC elements of T as one 16 B transaction
// ---------------------------------------------------------------------------

template <typename T>
struct VecIO;

template <>
struct VecIO<bf16_t> {
  static constexpr int V = 8;
  using vec_t = s8v;
  __device__ static void load(const bf16_t* p, float* out) {
    vec_t v = *(const vec_t*)p;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.s = v[j];
      out[j] = (float)u.b;
    }
  }
  __device__ static void store(bf16_t* p, const float* in) {
    vec_t v;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.b = (bf16_t)in[j];
      v[j] = u.s;
    }
    *(vec_t*)p = v;
  }
};

template <>
struct VecIO<float> {
  static constexpr int V = 4;
  using vec_t = f4v;
  __device__ static void load(const float* p, float* out) {
    f4v v = *(const f4v*)p;
    #pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = v[j];
  }
  __device__ static void store(float* p, const float* in) {
    f4v v;
    #pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = in[j];
    *(f4v*)p = v;
  }
};

// ---------------------------------------------------------------------------
// NHWC fast path — requires C % V == 0 and 2048 % C == 0 (fixed per-thread
// channel slots) and total < 2^31
// ---------------------------------------------------------------------------

// First channel of this thread's vectors. Vector i starts at channel
// (i*V) % C; it is the same for every i of the grid-stride loop because the
// launchers keep gridDim.x * 256 * V a multiple of C. One block row of 256*V
// elements is a multiple of C for every eligible C except fp32 C=2048, where
// it is half of C and the block index decides which half.
template <int V>
__device__ __forceinline__ u32 channel_slot(u32 C) {
  return ((blockIdx.x * blockDim.x + threadIdx.x) * (u32)V) % C;
}

// Per-channel shift the statistics are accumulated around: the mean of the
// channel's first n pixels, added up in index order by ONE thread, so that the
// stage-A kernels and stats_merge_finalize arrive at the same bits. n = 1 (the
// first pixel itself) on the fast path, where every thread needs the shift of
// its own channels; min(M, 32) on the generic path, where one thread per block
// computes it: the closer the shift is to the mean, the less E[d^2] exceeds
// the variance and the less of its rounding error the subtraction magnifies.
#define TFOSR_BN_SHIFT_PIXELS 32

template <typename T>
__device__ __forceinline__ float channel_shift(const T* __restrict__ x, int c,
                                               int C, long HW, bool nhwc,
                                               int n) {
  float s = 0.f;
  for (int m = 0; m < n; ++m)
    s += (float)x[nhwc ? (long)m * C + c : ((m / HW) * C + c) * HW + m % HW];
  return s / (float)n;
}

// Stage A: per-block partials into workspace[block][2C] via an LDS reduce —
// NO global atomics (a per-thread global-atomic tail serializes ~10^5 adds
// per channel address and was 40x slower than the loads themselves).
template <typename T>
__global__ void stats_nhwc_fast(const T* __restrict__ x,
                                float* __restrict__ partials, u32 nvec, u32 C) {
  extern __shared__ float lds[];  // [2C]: sums then sumsqs
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  float s[V], q[V], v[V], k[V];
  VecIO<T>::load(x + c0, k);  // shift: the first pixel of these channels
  #pragma unroll
  for (int j = 0; j < V; ++j) { s[j] = 0.f; q[j] = 0.f; }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(x + (size_t)i * V, v);
    #pragma unroll
    for (int j = 0; j < V; ++j) { float d = v[j] - k[j]; s[j] += d; q[j] += d * d; }
  }
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    atomicAdd(&lds[c0 + j], s[j]);
    atomicAdd(&lds[C + c0 + j], q[j]);
  }
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * 2 * C;
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) out[i] = lds[i];
}

// Stage B: sum partials over blocks + finalize mean/rstd + running stats.
// The partials are sums of (x - shift) and (x - shift)^2 with shift =
// channel_shift(..., nshift).
// One block per channel, 256 threads strided over the partial blocks — a
// single-block C-thread version serialized ~1000 loads per thread (227 us;
// 40x this kernel's data).
__global__ void stats_merge_finalize(const float* __restrict__ partials,
                                     int nblocks, u32 C,
                                     const void* __restrict__ x, int is_bf16,
                                     int is_nhwc, long HW, int nshift,
                                     float* __restrict__ save_mean,
                                     float* __restrict__ save_rstd,
                                     float* __restrict__ running_mean,
                                     float* __restrict__ running_var,
                                     long M, float momentum, float eps) {
  __shared__ float scratch[8];
  const u32 c = blockIdx.x;
  float s = 0.f, q = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    s += partials[(size_t)b * 2 * C + c];
    q += partials[(size_t)b * 2 * C + C + c];
  }
  s = block_sum<256>(s, scratch);
  __syncthreads();
  q = block_sum<256>(q, scratch);
  if (threadIdx.x != 0) return;
  const float shift =
      is_bf16 ? channel_shift((const bf16_t*)x, (int)c, (int)C, HW, is_nhwc, nshift)
              : channel_shift((const float*)x, (int)c, (int)C, HW, is_nhwc, nshift);
  float dmean = s / (float)M;
  float var = fmaxf(q / (float)M - dmean * dmean, 0.f);
  float mean = shift + dmean;
  save_mean[c] = mean;
  save_rstd[c] = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    float unbiased = (M > 1) ? var * (float)M / (float)(M - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// The same statistics from the tile partials that the GEMM / conv statistics
// epilogues leave behind (mfma_stats_epilogue.h): part[ntm][2][C], row t =
// (mean_t, M2_t) of the n_t = min(rows_per_tile, M - t * rows_per_tile) rows
// of tile t. Tiles combine by the parallel-variance formula, taken around the
// first tile's mean m0 so that the sums stay small where |mean| >> std:
//
//   mean = m0 + S1 / M,   S1 = sum n_t (mean_t - m0)
//   var  = (sum M2_t + S2) / M - (S1 / M)^2,   S2 = sum n_t (mean_t - m0)^2
//
// There are up to ~25 k tile rows (ResNet-50 layer1 at batch 1024), 3 % of the
// tensor's bytes, so the merge is two-level and reads coalesced over channels:
// a block is 64 channels x 4 row lanes; level 1 gives block (cx, k) the rows
// [k * chunk, (k + 1) * chunk) and writes ws[k][3][C] = (S1, S2, sum M2);
// level 2 sums the <= 256 rows of ws the same way and finalizes. Every sum
// has a fixed order.
#define TFOSR_TILE_MERGE_ROWS 256  // most rows of ws (level-1 blocks per column)

static inline int tile_merge_chunk(int ntm) {
  int chunk = (ntm + TFOSR_TILE_MERGE_ROWS - 1) / TFOSR_TILE_MERGE_ROWS;
  if (chunk < 32) chunk = 32;
  return (chunk + 3) / 4 * 4;
}

// sum over the 4 row lanes of a 64 x 4 block; valid in the threads of lane 0
__device__ __forceinline__ void tile_merge_lanes(float (&v)[3],
                                                 float (*lds)[4][64], u32 tx,
                                                 u32 ty) {
  #pragma unroll
  for (int j = 0; j < 3; ++j) lds[j][ty][tx] = v[j];
  __syncthreads();
  if (ty == 0) {
    #pragma unroll
    for (int j = 0; j < 3; ++j)
      v[j] = (lds[j][0][tx] + lds[j][1][tx]) + (lds[j][2][tx] + lds[j][3][tx]);
  }
}

__global__ void tile_stats_reduce(const float* __restrict__ part, int ntm, u32 C,
                                  int rows_per_tile, long M, int chunk,
                                  float* __restrict__ ws) {
  __shared__ float lds[3][4][64];
  const u32 tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const u32 c = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * chunk;
  const int r1 = r0 + chunk < ntm ? r0 + chunk : ntm;
  float v[3] = {0.f, 0.f, 0.f};
  if (c < C) {
    const float m0 = part[c];
    for (int r = r0 + (int)ty; r < r1; r += 4) {
      const float* p = part + (size_t)r * 2 * C;
      const long rem = M - (long)r * rows_per_tile;
      const float n = (float)(rem < rows_per_tile ? rem : rows_per_tile);
      const float d = p[c] - m0;
      v[0] += n * d;
      v[1] += n * d * d;
      v[2] += p[C + c];
    }
  }
  tile_merge_lanes(v, lds, tx, ty);
  if (ty == 0 && c < C) {
    float* out = ws + (size_t)blockIdx.y * 3 * C;
    out[c] = v[0];
    out[C + c] = v[1];
    out[2 * C + c] = v[2];
  }
}

__global__ void tile_stats_finalize(const float* __restrict__ ws, int nrows,
                                    u32 C, const float* __restrict__ part,
                                    float* __restrict__ save_mean,
                                    float* __restrict__ save_rstd,
                                    float* __restrict__ running_mean,
                                    float* __restrict__ running_var, long M,
                                    float momentum, float eps) {
  __shared__ float lds[3][4][64];
  const u32 tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const u32 c = blockIdx.x * 64 + tx;
  float v[3] = {0.f, 0.f, 0.f};
  if (c < C) {
    for (int r = (int)ty; r < nrows; r += 4) {
      const float* p = ws + (size_t)r * 3 * C;
      v[0] += p[c];
      v[1] += p[C + c];
      v[2] += p[2 * C + c];
    }
  }
  tile_merge_lanes(v, lds, tx, ty);
  if (ty != 0 || c >= C) return;
  const float dmean = v[0] / (float)M;
  const float var = fmaxf((v[2] + v[1]) / (float)M - dmean * dmean, 0.f);
  const float mean = part[c] + dmean;
  save_mean[c] = mean;
  save_rstd[c] = rsqrtf(var + eps);
  if (running_mean != nullptr) {
    float unbiased = (M > 1) ? var * (float)M / (float)(M - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// normalize (+add residual)(+relu); with RELU, also emit a per-element
// sign bitmask (1 byte per vector) so backward never re-reads y for gating
template <typename T, bool RELU, bool ADD>
__global__ void bn_apply_fast(const T* __restrict__ x, const T* __restrict__ res,
                              T* __restrict__ y, unsigned char* __restrict__ mask,
                              const float* __restrict__ mean,
                              const float* __restrict__ rstd,
                              const float* __restrict__ w,
                              const float* __restrict__ b, u32 nvec, u32 C) {
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  // (x - mean) * scale + bias: subtracting first keeps a channel with a tiny
  // variance (huge scale) exact where x*scale + (bias - mean*scale) cancels
  float sc[V], mu[V], sh[V], v[V], r[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    sc[j] = w[c0 + j] * rstd[c0 + j];
    mu[j] = mean[c0 + j];
    sh[j] = b[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(x + (size_t)i * V, v);
    if (ADD) VecIO<T>::load(res + (size_t)i * V, r);
    unsigned char m = 0;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float o = (v[j] - mu[j]) * sc[j] + sh[j];
      if (ADD) o += r[j];
      if (RELU) {
        if (o > 0.f) m |= (1u << j);
        o = fmaxf(o, 0.f);
      }
      v[j] = o;
    }
    VecIO<T>::store(y + (size_t)i * V, v);
    if (RELU && mask != nullptr) mask[i] = m;
  }
}

// backward reductions: g = dy * gate(y); dbeta += g; dgamma += g * xhat;
// optionally write g out (the residual branch gradient for the ADD variant)
template <typename T, bool RELU, bool WRITE_G>
__global__ void bwd_stats_fast(const T* __restrict__ x, const T* __restrict__ dy,
                               const unsigned char* __restrict__ mask,
                               T* __restrict__ gout,
                               const float* __restrict__ mean,
                               const float* __restrict__ rstd,
                               float* __restrict__ partials, u32 nvec, u32 C) {
  extern __shared__ float lds[];  // [2C]: dgamma then dbeta
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  float sg[V], sb[V], xv[V], dv[V];
  float mu[V], rs[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    sg[j] = 0.f; sb[j] = 0.f;
    mu[j] = mean[c0 + j]; rs[j] = rstd[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(x + (size_t)i * V, xv);
    VecIO<T>::load(dy + (size_t)i * V, dv);
    unsigned char m = RELU ? mask[i] : 0;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = RELU ? (((m >> j) & 1) ? dv[j] : 0.f) : dv[j];
      sb[j] += g;
      sg[j] += g * (xv[j] - mu[j]) * rs[j];
      dv[j] = g;
    }
    if (WRITE_G) VecIO<T>::store(gout + (size_t)i * V, dv);
  }
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    atomicAdd(&lds[c0 + j], sg[j]);
    atomicAdd(&lds[C + c0 + j], sb[j]);
  }
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * 2 * C;
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) out[i] = lds[i];
}

__global__ void bwd_stats_merge(const float* __restrict__ partials, int nblocks,
                                u32 C, float* __restrict__ dg,
                                float* __restrict__ db) {
  __shared__ float scratch[8];
  const u32 c = blockIdx.x;
  float sg = 0.f, sb = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    sg += partials[(size_t)b * 2 * C + c];
    sb += partials[(size_t)b * 2 * C + C + c];
  }
  sg = block_sum<256>(sg, scratch);
  __syncthreads();
  sb = block_sum<256>(sb, scratch);
  if (threadIdx.x == 0) {
    dg[c] = sg;
    db[c] = sb;
  }
}

// dx = w*rstd * (g - db/M - xhat * dg/M); g recomputed from (dy, y) or read
// from the gated gradient written by bwd_stats (GATED=false).
template <typename T, bool RELU>
__global__ void bwd_dx_fast(const T* __restrict__ x, const T* __restrict__ dy,
                            const unsigned char* __restrict__ mask,
                            T* __restrict__ dx,
                            const float* __restrict__ mean,
                            const float* __restrict__ rstd,
                            const float* __restrict__ w,
                            const float* __restrict__ dg,
                            const float* __restrict__ db,
                            u32 nvec, u32 C, float invM) {
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  float sc[V], mu[V], rs[V], dgm[V], dbm[V], xv[V], dv[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    mu[j] = mean[c0 + j]; rs[j] = rstd[c0 + j];
    sc[j] = w[c0 + j] * rs[j];
    dgm[j] = dg[c0 + j] * invM;
    dbm[j] = db[c0 + j] * invM;
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(x + (size_t)i * V, xv);
    VecIO<T>::load(dy + (size_t)i * V, dv);
    unsigned char m = RELU ? mask[i] : 0;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = RELU ? (((m >> j) & 1) ? dv[j] : 0.f) : dv[j];
      float xhat = (xv[j] - mu[j]) * rs[j];
      dv[j] = sc[j] * (g - dbm[j] - xhat * dgm[j]);
    }
    VecIO<T>::store(dx + (size_t)i * V, dv);
  }
}

// ---------------------------------------------------------------------------
// The join of two BatchNorms, y = relu(bn_a(xa) + bn_b(xb)): the tail of a
// residual block whose shortcut ends in a BN of its own (a: the main branch,
// b: the downsample branch). As two calls, the normalized shortcut is written
// and read back in forward, and in backward the gated gradient is written
// once and read three times; here each of xa, xb, dy is read once per pass.
// Same layout rules, channel slots and mask format as the kernels above.
// ---------------------------------------------------------------------------

template <typename T>
__global__ void bn_apply_dual_fast(const T* __restrict__ xa,
                                   const T* __restrict__ xb, T* __restrict__ y,
                                   unsigned char* __restrict__ mask,
                                   const float* __restrict__ mean_a,
                                   const float* __restrict__ rstd_a,
                                   const float* __restrict__ w_a,
                                   const float* __restrict__ b_a,
                                   const float* __restrict__ mean_b,
                                   const float* __restrict__ rstd_b,
                                   const float* __restrict__ w_b,
                                   const float* __restrict__ b_b,
                                   u32 nvec, u32 C) {
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  float sca[V], mua[V], sha[V], scb[V], mub[V], shb[V], va[V], vb[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    sca[j] = w_a[c0 + j] * rstd_a[c0 + j];
    mua[j] = mean_a[c0 + j];
    sha[j] = b_a[c0 + j];
    scb[j] = w_b[c0 + j] * rstd_b[c0 + j];
    mub[j] = mean_b[c0 + j];
    shb[j] = b_b[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(xa + (size_t)i * V, va);
    VecIO<T>::load(xb + (size_t)i * V, vb);
    unsigned char m = 0;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      // each branch as bn_apply_fast computes it; the shortcut is not rounded
      // to T before the add
      float o = (va[j] - mua[j]) * sca[j] + sha[j];
      o += (vb[j] - mub[j]) * scb[j] + shb[j];
      if (o > 0.f) m |= (1u << j);
      va[j] = fmaxf(o, 0.f);
    }
    VecIO<T>::store(y + (size_t)i * V, va);
    mask[i] = m;
  }
}

// g = dy gated by the mask; dgamma_a += g * xhat_a; dgamma_b += g * xhat_b;
// dbeta += g (the same sum for both BNs): partials[block][3C]
template <typename T>
__global__ void bwd_stats_dual_fast(const T* __restrict__ xa,
                                    const T* __restrict__ xb,
                                    const T* __restrict__ dy,
                                    const unsigned char* __restrict__ mask,
                                    const float* __restrict__ mean_a,
                                    const float* __restrict__ rstd_a,
                                    const float* __restrict__ mean_b,
                                    const float* __restrict__ rstd_b,
                                    float* __restrict__ partials, u32 nvec,
                                    u32 C) {
  extern __shared__ float lds[];  // [3C]: dgamma_a, dgamma_b, dbeta
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  for (u32 i = threadIdx.x; i < 3 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  float sga[V], sgb[V], sb[V], av[V], bv[V], dv[V];
  float mua[V], rsa[V], mub[V], rsb[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    sga[j] = 0.f; sgb[j] = 0.f; sb[j] = 0.f;
    mua[j] = mean_a[c0 + j]; rsa[j] = rstd_a[c0 + j];
    mub[j] = mean_b[c0 + j]; rsb[j] = rstd_b[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(xa + (size_t)i * V, av);
    VecIO<T>::load(xb + (size_t)i * V, bv);
    VecIO<T>::load(dy + (size_t)i * V, dv);
    unsigned char m = mask[i];
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = ((m >> j) & 1) ? dv[j] : 0.f;
      sb[j] += g;
      sga[j] += g * (av[j] - mua[j]) * rsa[j];
      sgb[j] += g * (bv[j] - mub[j]) * rsb[j];
    }
  }
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    atomicAdd(&lds[c0 + j], sga[j]);
    atomicAdd(&lds[C + c0 + j], sgb[j]);
    atomicAdd(&lds[2 * C + c0 + j], sb[j]);
  }
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * 3 * C;
  for (u32 i = threadIdx.x; i < 3 * C; i += blockDim.x) out[i] = lds[i];
}

// the shared dbeta goes to both BNs' outputs
__global__ void bwd_stats_dual_merge(const float* __restrict__ partials,
                                     int nblocks, u32 C,
                                     float* __restrict__ dg_a,
                                     float* __restrict__ dg_b,
                                     float* __restrict__ db_a,
                                     float* __restrict__ db_b) {
  __shared__ float scratch[8];
  const u32 c = blockIdx.x;
  float sa = 0.f, sg = 0.f, sb = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) {
    sa += partials[(size_t)b * 3 * C + c];
    sg += partials[(size_t)b * 3 * C + C + c];
    sb += partials[(size_t)b * 3 * C + 2 * C + c];
  }
  sa = block_sum<256>(sa, scratch);
  __syncthreads();
  sg = block_sum<256>(sg, scratch);
  __syncthreads();
  sb = block_sum<256>(sb, scratch);
  if (threadIdx.x == 0) {
    dg_a[c] = sa;
    dg_b[c] = sg;
    db_a[c] = sb;
    db_b[c] = sb;
  }
}

// dxa and dxb as bwd_dx_fast computes each, from one read of dy and the mask
template <typename T>
__global__ void bwd_dx_dual_fast(const T* __restrict__ xa,
                                 const T* __restrict__ xb,
                                 const T* __restrict__ dy,
                                 const unsigned char* __restrict__ mask,
                                 T* __restrict__ dxa, T* __restrict__ dxb,
                                 const float* __restrict__ mean_a,
                                 const float* __restrict__ rstd_a,
                                 const float* __restrict__ w_a,
                                 const float* __restrict__ dg_a,
                                 const float* __restrict__ mean_b,
                                 const float* __restrict__ rstd_b,
                                 const float* __restrict__ w_b,
                                 const float* __restrict__ dg_b,
                                 const float* __restrict__ db,
                                 u32 nvec, u32 C, float invM) {
  constexpr int V = VecIO<T>::V;
  const u32 c0 = channel_slot<V>(C);
  float sca[V], mua[V], rsa[V], dga[V], scb[V], mub[V], rsb[V], dgb[V], dbm[V];
  float av[V], bv[V], dv[V];
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    mua[j] = mean_a[c0 + j]; rsa[j] = rstd_a[c0 + j];
    sca[j] = w_a[c0 + j] * rsa[j];
    dga[j] = dg_a[c0 + j] * invM;
    mub[j] = mean_b[c0 + j]; rsb[j] = rstd_b[c0 + j];
    scb[j] = w_b[c0 + j] * rsb[j];
    dgb[j] = dg_b[c0 + j] * invM;
    dbm[j] = db[c0 + j] * invM;
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    VecIO<T>::load(xa + (size_t)i * V, av);
    VecIO<T>::load(xb + (size_t)i * V, bv);
    VecIO<T>::load(dy + (size_t)i * V, dv);
    unsigned char m = mask[i];
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float g = ((m >> j) & 1) ? dv[j] : 0.f;
      float xhat_a = (av[j] - mua[j]) * rsa[j];
      float xhat_b = (bv[j] - mub[j]) * rsb[j];
      av[j] = sca[j] * (g - dbm[j] - xhat_a * dga[j]);
      bv[j] = scb[j] * (g - dbm[j] - xhat_b * dgb[j]);
    }
    VecIO<T>::store(dxa + (size_t)i * V, av);
    VecIO<T>::store(dxb + (size_t)i * V, bv);
  }
}

// ---------------------------------------------------------------------------
// Generic fallbacks (any layout/shape): scalar, 64-bit safe
// ---------------------------------------------------------------------------

// The generic reductions give block (c, k) the pixels [k*CHUNK, (k+1)*CHUNK) of
// channel c (further chunks by grid stride): a register chain of CHUNK/256
// adds per thread, a tree over the block, then ONE atomic per block and
// channel into the zeroed workspace. An atomic per element made every channel
// sum a serial fp32 chain of M adds, whose rounding error grows with M.
#define TFOSR_BN_CHUNK 4096

template <bool NHWC>
__device__ __forceinline__ long pixel_index(long m, int c, int C, long HW) {
  return NHWC ? m * C + c : ((m / HW) * C + c) * HW + m % HW;
}

static inline dim3 generic_red_grid(long M, int C) {
  long chunks = (M + TFOSR_BN_CHUNK - 1) / TFOSR_BN_CHUNK;
  if (chunks > 1024) chunks = 1024;
  return dim3((unsigned)C, (unsigned)(chunks > 0 ? chunks : 1));
}

template <typename T, bool NHWC>
__global__ void stats_generic(const T* __restrict__ x, float* __restrict__ ws,
                              long M, int C, long HW) {
  __shared__ float scratch[8];
  __shared__ float shift;
  const int c = blockIdx.x;
  if (threadIdx.x == 0)
    shift = channel_shift(x, c, C, HW, NHWC,
                          M < TFOSR_BN_SHIFT_PIXELS ? (int)M : TFOSR_BN_SHIFT_PIXELS);
  __syncthreads();
  const float k = shift;
  float s = 0.f, q = 0.f;
  for (long m0 = (long)blockIdx.y * TFOSR_BN_CHUNK; m0 < M;
       m0 += (long)gridDim.y * TFOSR_BN_CHUNK) {
    const long m1 = m0 + TFOSR_BN_CHUNK < M ? m0 + TFOSR_BN_CHUNK : M;
    for (long m = m0 + threadIdx.x; m < m1; m += blockDim.x) {
      float d = (float)x[pixel_index<NHWC>(m, c, C, HW)] - k;
      s += d;
      q += d * d;
    }
  }
  s = block_sum<256>(s, scratch);
  __syncthreads();
  q = block_sum<256>(q, scratch);
  if (threadIdx.x == 0) {
    atomicAdd(&ws[c], s);
    atomicAdd(&ws[C + c], q);
  }
}

template <typename T, bool NHWC, bool RELU, bool ADD>
__global__ void bn_apply_generic(const T* __restrict__ x, const T* __restrict__ res,
                                 T* __restrict__ y,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 const float* __restrict__ w,
                                 const float* __restrict__ b,
                                 long total, int C, long HW) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    int c = NHWC ? (int)(idx % C) : (int)((idx / HW) % C);
    float o = ((float)x[idx] - mean[c]) * rstd[c] * w[c] + b[c];
    if (ADD) o += (float)res[idx];
    if (RELU) o = fmaxf(o, 0.f);
    y[idx] = (T)o;
  }
}

template <typename T, bool NHWC, bool RELU, bool WRITE_G>
__global__ void bwd_stats_generic(const T* __restrict__ x, const T* __restrict__ dy,
                                  const T* __restrict__ y, T* __restrict__ gout,
                                  const float* __restrict__ mean,
                                  const float* __restrict__ rstd,
                                  float* __restrict__ ws,
                                  long M, int C, long HW) {
  __shared__ float scratch[8];
  const int c = blockIdx.x;
  const float mu = mean[c], rs = rstd[c];
  float sg = 0.f, sb = 0.f;
  for (long m0 = (long)blockIdx.y * TFOSR_BN_CHUNK; m0 < M;
       m0 += (long)gridDim.y * TFOSR_BN_CHUNK) {
    const long m1 = m0 + TFOSR_BN_CHUNK < M ? m0 + TFOSR_BN_CHUNK : M;
    for (long m = m0 + threadIdx.x; m < m1; m += blockDim.x) {
      const long idx = pixel_index<NHWC>(m, c, C, HW);
      float g = (float)dy[idx];
      if (RELU) g = ((float)y[idx] > 0.f) ? g : 0.f;
      sb += g;
      sg += g * ((float)x[idx] - mu) * rs;
      if (WRITE_G) gout[idx] = (T)g;
    }
  }
  sg = block_sum<256>(sg, scratch);
  __syncthreads();
  sb = block_sum<256>(sb, scratch);
  if (threadIdx.x == 0) {
    atomicAdd(&ws[c], sg);
    atomicAdd(&ws[C + c], sb);
  }
}

template <typename T, bool NHWC, bool RELU>
__global__ void bwd_dx_generic(const T* __restrict__ x, const T* __restrict__ dy,
                               const T* __restrict__ y, T* __restrict__ dx,
                               const float* __restrict__ mean,
                               const float* __restrict__ rstd,
                               const float* __restrict__ w,
                               const float* __restrict__ dg,
                               const float* __restrict__ db,
                               long total, int C, long HW, float invM) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    int c = NHWC ? (int)(idx % C) : (int)((idx / HW) % C);
    float g = (float)dy[idx];
    if (RELU) g = ((float)y[idx] > 0.f) ? g : 0.f;
    float xhat = ((float)x[idx] - mean[c]) * rstd[c];
    dx[idx] = (T)(w[c] * rstd[c] * (g - db[c] * invM - xhat * dg[c] * invM));
  }
}


// ---------------------------------------------------------------------------
// extern "C" launchers — dispatch fast path when eligible
// ---------------------------------------------------------------------------

static inline bool fast_ok(int is_nhwc, long total, int C, int vec) {
  return is_nhwc && total < (1L << 31) && C % vec == 0 && 2048 % C == 0;
}

// The fast kernels need gridDim.x * 256 * vec to be a multiple of C so that a
// thread's channel slot survives the grid stride: grids are multiples of this
// (1 for every eligible shape except fp32 C=2048, where it is 2).
static inline int grid_quantum(int C, int vec) {
  int row = 256 * vec;
  return C > row ? C / row : 1;
}

static inline int fast_grid(long nvec, int quantum) {
  long g = (nvec + 255) / 256;
  g = (g + quantum - 1) / quantum * quantum;
  if (g > TFOSR_MAX_GRID) g = TFOSR_MAX_GRID;  // a multiple of every quantum
  return (int)(g > 0 ? g : quantum);
}

static inline int red_grid(long nvec, int quantum) {
  // reduction stage A: >=32 vectors per thread bounds the partials traffic
  // to ~3% of the tensor; [64, 1024] keeps the chip busy on small layers
  long g = nvec / (256 * 32);
  if (g < 64) g = 64;
  if (g > 1024) g = 1024;
  g -= g % quantum;
  return (int)g;
}

extern "C" {

// #blocks the two-stage fast reduction will use; 0 => generic path
// (caller sizes the partials workspace as max(nb,1) * 2C floats and must
// ZERO it when nb == 0)
int tfosr_bn_fast_blocks(long total, int C, int is_bf16, int is_nhwc) {
  int vec = is_bf16 ? 8 : 4;
  if (!fast_ok(is_nhwc, total, C, vec)) return 0;
  return red_grid(total / vec, grid_quantum(C, vec));
}

void tfosr_bn_stats(const void* x, int is_bf16, int is_nhwc, float* partials,
                    int nb, int N, int C, long HW, hipStream_t s) {
  const long total = (long)N * HW * C;
  if (nb > 0) {
    int vec = is_bf16 ? 8 : 4;
    u32 nvec = (u32)(total / vec);
    size_t lds = 2 * (size_t)C * sizeof(float);
    if (is_bf16)
      hipLaunchKernelGGL(stats_nhwc_fast<bf16_t>, dim3(nb), dim3(256), lds, s,
                         (const bf16_t*)x, partials, nvec, (u32)C);
    else
      hipLaunchKernelGGL(stats_nhwc_fast<float>, dim3(nb), dim3(256), lds, s,
                         (const float*)x, partials, nvec, (u32)C);
    return;
  }
  const long M = (long)N * HW;
  dim3 grid = generic_red_grid(M, C);
#define SG(T, L) hipLaunchKernelGGL((stats_generic<T, L>), grid, dim3(256), \
                                    0, s, (const T*)x, partials, M, C, HW)
  if (is_bf16) { if (is_nhwc) SG(bf16_t, true); else SG(bf16_t, false); }
  else { if (is_nhwc) SG(float, true); else SG(float, false); }
#undef SG
}

// x, is_bf16, is_nhwc, HW: as given to tfosr_bn_stats (locates the shift)
void tfosr_bn_finalize(const float* partials, int nb, const void* x,
                       int is_bf16, int is_nhwc, long HW, float* save_mean,
                       float* save_rstd, float* running_mean, float* running_var,
                       long M, int C, float momentum, float eps, hipStream_t s) {
  hipLaunchKernelGGL(stats_merge_finalize, dim3(C), dim3(256), 0, s,
                     partials, nb > 0 ? nb : 1, (u32)C, x, is_bf16, is_nhwc, HW,
                     nb > 0 ? 1 : (int)(M < TFOSR_BN_SHIFT_PIXELS ? M : TFOSR_BN_SHIFT_PIXELS),
                     save_mean, save_rstd,
                     running_mean, running_var, M, momentum, eps);
}

// rows of the level-1 workspace tfosr_bn_tile_finalize() needs for ntm tile
// rows: ws holds rows * 3C floats
int tfosr_bn_tile_ws_rows(int ntm) {
  const int chunk = tile_merge_chunk(ntm);
  return (ntm + chunk - 1) / chunk;
}

// tfosr_bn_stats + tfosr_bn_finalize from the tile partials part[ntm][2][C] of
// a GEMM / conv statistics epilogue instead of from the tensor
void tfosr_bn_tile_finalize(const float* part, int ntm, int rows_per_tile,
                            float* ws, float* save_mean, float* save_rstd,
                            float* running_mean, float* running_var, long M,
                            int C, float momentum, float eps, hipStream_t s) {
  const int chunk = tile_merge_chunk(ntm);
  const int nrows = (ntm + chunk - 1) / chunk;
  const int cgroups = (C + 63) / 64;
  hipLaunchKernelGGL(tile_stats_reduce, dim3(cgroups, nrows), dim3(256), 0, s,
                     part, ntm, (u32)C, rows_per_tile, M, chunk, ws);
  hipLaunchKernelGGL(tile_stats_finalize, dim3(cgroups), dim3(256), 0, s, ws,
                     nrows, (u32)C, part, save_mean, save_rstd, running_mean,
                     running_var, M, momentum, eps);
}

// relu: 0/1; res: nullptr for plain BN; mask: sign bits out (fast path only)
void tfosr_bn_apply(const void* x, const void* res, void* y, unsigned char* mask,
                    const float* mean,
                    const float* rstd, const float* w, const float* b,
                    int is_bf16, int is_nhwc, int relu, long total, int C,
                    long HW, hipStream_t s) {
  int vec = is_bf16 ? 8 : 4;
  const bool add = res != nullptr;
  if (fast_ok(is_nhwc, total, C, vec)) {
    u32 nvec = (u32)(total / vec);
    int grid = fast_grid(nvec, grid_quantum(C, vec));
#define APPLY_FAST(T, R, A) \
    hipLaunchKernelGGL((bn_apply_fast<T, R, A>), dim3(grid), dim3(256), 0, s, \
                       (const T*)x, (const T*)res, (T*)y, mask, mean, rstd, w, b, \
                       nvec, (u32)C)
    if (is_bf16) {
      if (relu) { if (add) APPLY_FAST(bf16_t, true, true); else APPLY_FAST(bf16_t, true, false); }
      else      { if (add) APPLY_FAST(bf16_t, false, true); else APPLY_FAST(bf16_t, false, false); }
    } else {
      if (relu) { if (add) APPLY_FAST(float, true, true); else APPLY_FAST(float, true, false); }
      else      { if (add) APPLY_FAST(float, false, true); else APPLY_FAST(float, false, false); }
    }
#undef APPLY_FAST
    return;
  }
  int grid = tfosr_grid(total, 256);
#define APPLY_GEN(T, L, R, A) \
  hipLaunchKernelGGL((bn_apply_generic<T, L, R, A>), dim3(grid), dim3(256), 0, s, \
                     (const T*)x, (const T*)res, (T*)y, mean, rstd, w, b, \
                     total, C, HW)
  if (is_bf16) {
    if (is_nhwc) { if (relu) { if (add) APPLY_GEN(bf16_t, true, true, true); else APPLY_GEN(bf16_t, true, true, false); }
                   else { if (add) APPLY_GEN(bf16_t, true, false, true); else APPLY_GEN(bf16_t, true, false, false); } }
    else { if (relu) { if (add) APPLY_GEN(bf16_t, false, true, true); else APPLY_GEN(bf16_t, false, true, false); }
           else { if (add) APPLY_GEN(bf16_t, false, false, true); else APPLY_GEN(bf16_t, false, false, false); } }
  } else {
    if (is_nhwc) { if (relu) { if (add) APPLY_GEN(float, true, true, true); else APPLY_GEN(float, true, true, false); }
                   else { if (add) APPLY_GEN(float, true, false, true); else APPLY_GEN(float, true, false, false); } }
    else { if (relu) { if (add) APPLY_GEN(float, false, true, true); else APPLY_GEN(float, false, true, false); }
           else { if (add) APPLY_GEN(float, false, false, true); else APPLY_GEN(float, false, false, false); } }
  }
#undef APPLY_GEN
}

// gout: non-null => also write gated upstream grad (residual-branch gradient)
// fast path gates from `mask` (written by apply); generic path gates from y
void tfosr_bn_bwd_stats(const void* x, const void* dy, const void* y,
                        const unsigned char* mask, void* gout,
                        const float* mean, const float* rstd, float* partials,
                        int nb, int is_bf16, int is_nhwc, int relu, int N, int C,
                        long HW, hipStream_t s) {
  const long total = (long)N * HW * C;
  const bool wg = gout != nullptr;
  if (nb > 0) {
    int vec = is_bf16 ? 8 : 4;
    u32 nvec = (u32)(total / vec);
    size_t lds = 2 * (size_t)C * sizeof(float);
#define BS_FAST(T, R, W) \
    hipLaunchKernelGGL((bwd_stats_fast<T, R, W>), dim3(nb), dim3(256), lds, s, \
                       (const T*)x, (const T*)dy, mask, (T*)gout, \
                       mean, rstd, partials, nvec, (u32)C)
    if (is_bf16) {
      if (relu) { if (wg) BS_FAST(bf16_t, true, true); else BS_FAST(bf16_t, true, false); }
      else      { if (wg) BS_FAST(bf16_t, false, true); else BS_FAST(bf16_t, false, false); }
    } else {
      if (relu) { if (wg) BS_FAST(float, true, true); else BS_FAST(float, true, false); }
      else      { if (wg) BS_FAST(float, false, true); else BS_FAST(float, false, false); }
    }
#undef BS_FAST
    return;
  }
  const long M = (long)N * HW;
  dim3 grid = generic_red_grid(M, C);
#define BS_GEN(T, L, R, W) \
  hipLaunchKernelGGL((bwd_stats_generic<T, L, R, W>), grid, dim3(256), 0, s, \
                     (const T*)x, (const T*)dy, (const T*)y, (T*)gout, \
                     mean, rstd, partials, M, C, HW)
  if (is_bf16) {
    if (is_nhwc) { if (relu) { if (wg) BS_GEN(bf16_t, true, true, true); else BS_GEN(bf16_t, true, true, false); }
                   else { if (wg) BS_GEN(bf16_t, true, false, true); else BS_GEN(bf16_t, true, false, false); } }
    else { if (relu) { if (wg) BS_GEN(bf16_t, false, true, true); else BS_GEN(bf16_t, false, true, false); }
           else { if (wg) BS_GEN(bf16_t, false, false, true); else BS_GEN(bf16_t, false, false, false); } }
  } else {
    if (is_nhwc) { if (relu) { if (wg) BS_GEN(float, true, true, true); else BS_GEN(float, true, true, false); }
                   else { if (wg) BS_GEN(float, true, false, true); else BS_GEN(float, true, false, false); } }
    else { if (relu) { if (wg) BS_GEN(float, false, true, true); else BS_GEN(float, false, true, false); }
           else { if (wg) BS_GEN(float, false, false, true); else BS_GEN(float, false, false, false); } }
  }
#undef BS_GEN
}

void tfosr_bn_bwd_merge(const float* partials, int nb, float* dg, float* db,
                        int C, hipStream_t s) {
  hipLaunchKernelGGL(bwd_stats_merge, dim3(C), dim3(256), 0, s,
                     partials, nb > 0 ? nb : 1, (u32)C, dg, db);
}

void tfosr_bn_bwd_dx(const void* x, const void* dy, const void* y,
                     const unsigned char* mask,
                     const float* mean, const float* rstd, const float* w,
                     const float* dg, const float* db, void* dx, int is_bf16,
                     int is_nhwc, int relu, long total, int C, long HW,
                     hipStream_t s) {
  const float invM = 1.f / (float)(total / C);
  int vec = is_bf16 ? 8 : 4;
  if (fast_ok(is_nhwc, total, C, vec)) {
    u32 nvec = (u32)(total / vec);
    int grid = fast_grid(nvec, grid_quantum(C, vec));
#define DX_FAST(T, R) \
    hipLaunchKernelGGL((bwd_dx_fast<T, R>), dim3(grid), dim3(256), 0, s, \
                       (const T*)x, (const T*)dy, mask, (T*)dx, \
                       mean, rstd, w, dg, db, nvec, (u32)C, invM)
    if (is_bf16) { if (relu) DX_FAST(bf16_t, true); else DX_FAST(bf16_t, false); }
    else { if (relu) DX_FAST(float, true); else DX_FAST(float, false); }
#undef DX_FAST
    return;
  }
  int grid = tfosr_grid(total, 256);
#define DX_GEN(T, L, R) \
  hipLaunchKernelGGL((bwd_dx_generic<T, L, R>), dim3(grid), dim3(256), 0, s, \
                     (const T*)x, (const T*)dy, (const T*)y, (T*)dx, \
                     mean, rstd, w, dg, db, total, C, HW, invM)
  if (is_bf16) {
    if (is_nhwc) { if (relu) DX_GEN(bf16_t, true, true); else DX_GEN(bf16_t, true, false); }
    else { if (relu) DX_GEN(bf16_t, false, true); else DX_GEN(bf16_t, false, false); }
  } else {
    if (is_nhwc) { if (relu) DX_GEN(float, true, true); else DX_GEN(float, true, false); }
    else { if (relu) DX_GEN(float, false, true); else DX_GEN(float, false, false); }
  }
#undef DX_GEN
}

// The dual (two-BN join) launchers: NHWC fast path only, nb from
// tfosr_bn_fast_blocks() must be > 0; the partials hold nb * 3C floats.

void tfosr_bn_apply_dual(const void* xa, const void* xb, void* y,
                         unsigned char* mask, const float* mean_a,
                         const float* rstd_a, const float* w_a,
                         const float* b_a, const float* mean_b,
                         const float* rstd_b, const float* w_b,
                         const float* b_b, int is_bf16, long total, int C,
                         hipStream_t s) {
  int vec = is_bf16 ? 8 : 4;
  u32 nvec = (u32)(total / vec);
  int grid = fast_grid(nvec, grid_quantum(C, vec));
#define APPLY_DUAL(T) \
  hipLaunchKernelGGL((bn_apply_dual_fast<T>), dim3(grid), dim3(256), 0, s, \
                     (const T*)xa, (const T*)xb, (T*)y, mask, mean_a, rstd_a, \
                     w_a, b_a, mean_b, rstd_b, w_b, b_b, nvec, (u32)C)
  if (is_bf16) APPLY_DUAL(bf16_t); else APPLY_DUAL(float);
#undef APPLY_DUAL
}

void tfosr_bn_bwd_stats_dual(const void* xa, const void* xb, const void* dy,
                             const unsigned char* mask, const float* mean_a,
                             const float* rstd_a, const float* mean_b,
                             const float* rstd_b, float* partials, int nb,
                             int is_bf16, long total, int C, hipStream_t s) {
  int vec = is_bf16 ? 8 : 4;
  u32 nvec = (u32)(total / vec);
  size_t lds = 3 * (size_t)C * sizeof(float);
#define BS_DUAL(T) \
  hipLaunchKernelGGL((bwd_stats_dual_fast<T>), dim3(nb), dim3(256), lds, s, \
                     (const T*)xa, (const T*)xb, (const T*)dy, mask, mean_a, \
                     rstd_a, mean_b, rstd_b, partials, nvec, (u32)C)
  if (is_bf16) BS_DUAL(bf16_t); else BS_DUAL(float);
#undef BS_DUAL
}

void tfosr_bn_bwd_merge_dual(const float* partials, int nb, float* dg_a,
                             float* dg_b, float* db_a, float* db_b, int C,
                             hipStream_t s) {
  hipLaunchKernelGGL(bwd_stats_dual_merge, dim3(C), dim3(256), 0, s,
                     partials, nb, (u32)C, dg_a, dg_b, db_a, db_b);
}

void tfosr_bn_bwd_dx_dual(const void* xa, const void* xb, const void* dy,
                          const unsigned char* mask, void* dxa, void* dxb,
                          const float* mean_a, const float* rstd_a,
                          const float* w_a, const float* dg_a,
                          const float* mean_b, const float* rstd_b,
                          const float* w_b, const float* dg_b, const float* db,
                          int is_bf16, long total, int C, hipStream_t s) {
  const float invM = 1.f / (float)(total / C);
  int vec = is_bf16 ? 8 : 4;
  u32 nvec = (u32)(total / vec);
  int grid = fast_grid(nvec, grid_quantum(C, vec));
#define DX_DUAL(T) \
  hipLaunchKernelGGL((bwd_dx_dual_fast<T>), dim3(grid), dim3(256), 0, s, \
                     (const T*)xa, (const T*)xb, (const T*)dy, mask, (T*)dxa, \
                     (T*)dxb, mean_a, rstd_a, w_a, dg_a, mean_b, rstd_b, w_b, \
                     dg_b, db, nvec, (u32)C, invM)
  if (is_bf16) DX_DUAL(bf16_t); else DX_DUAL(float);
#undef DX_DUAL
}

}  // extern "C"
