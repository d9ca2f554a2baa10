// Dense softmax cross-entropy for gfx950 with ignore_index, label smoothing
// and a range-checked target.
//
//   loss_i    = lse_i - (1-eps) * x[i, t_i] - (eps/C) * sum_c x[i, c]
//   dlogits   = (exp(x - lse_i) - (1-eps) * [c == t_i] - eps/C) * g_i
//
// A row whose target equals ignore_index, or lies outside [0, C), contributes
// zero loss and zero gradient; no kernel indexes logits with such a target.
// All arithmetic is fp32; lse is saved per row and backward recomputes the
// softmax from it.
//
// Three families, chosen by the bindings from layout and C:
//   rows     class-contiguous rows, C >= 64: one block per row
//   strided  standard-contiguous (N, C, S): a lane owns 1 (scalar) or V
//            consecutive pixels (16 B loads) and walks the classes at stride S
//            with an online max/sum
//   tile     class-contiguous rows, C < 64: R rows (R*C contiguous elements)
//            staged through LDS with 16 B loads, one lane reduces one row;
//            the fp32 LDS rows have an odd dword stride so the per-lane row
//            walk hits 64 different banks
//
// Reductions: every block writes one (loss_sum, n_valid) partial and a
// single-block finalize adds them in a fixed order; no floating-point
// atomics, so equal inputs give equal bits.
#include "tfosr_common.h"

namespace {

template <typename T>
struct XVec;

template <>
struct XVec<bf16_t> {
  static constexpr int V = 8;
  __device__ static void load(const bf16_t* p, float* out) {
    s8v v = *(const s8v*)p;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.s = v[j];
      out[j] = (float)u.b;
    }
  }
  __device__ static void store(bf16_t* p, const float* in) {
    s8v v;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.b = (bf16_t)in[j];
      v[j] = u.s;
    }
    *(s8v*)p = v;
  }
};

template <>
struct XVec<float> {
  static constexpr int V = 4;
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

struct XentArgs {
  long ignore_index;
  float eps;        // label smoothing
  int C;
};

__device__ __forceinline__ bool target_ok(long t, const XentArgs& a) {
  return t != a.ignore_index && t >= 0 && t < (long)a.C;
}

__device__ __forceinline__ float row_loss(float lse, float xt, float sumx,
                                          const XentArgs& a) {
  if (a.eps == 0.f) return lse - xt;
  return lse - (1.f - a.eps) * xt - (a.eps / (float)a.C) * sumx;
}

// Upstream gradient: a per-row vector (reduction none) or a device scalar,
// divided in-kernel by max(n_valid, 1) for the mean.
struct XentGrad {
  const float* rows;
  const float* scalar;
  const int* nvalid;
  int mean;
};

__device__ __forceinline__ float grad_scale(const XentGrad& g) {
  if (g.rows) return 1.f;
  float s = g.scalar[0];
  if (g.mean) {
    int n = g.nvalid[0];
    s = s / (float)(n > 1 ? n : 1);
  }
  return s;
}

// The loss sum is carried as an unevaluated fp32 pair (hi, lo) and every add
// is an error-free TwoSum, so the reduced loss is the row losses' sum rounded
// once, whatever the grid and the order of the adds.
__device__ __forceinline__ void sum2_add(float& hi, float& lo, float bh,
                                         float bl) {
  float s = hi + bh;
  float bb = s - hi;
  float err = (hi - (s - bb)) + (bh - bb);
  hi = s;
  lo += err + bl;
}

// (loss pair, count) block reduction in a fixed order; result valid in
// thread 0. Call from uniform control flow; blockDim.x is a multiple of 64.
__device__ __forceinline__ void block_sum2(float& hi, float& lo, int& n) {
  __shared__ float sh[16], sl[16];
  __shared__ int si[16];
  for (int off = 32; off > 0; off >>= 1) {
    float oh = __shfl_down(hi, off, 64);
    float ol = __shfl_down(lo, off, 64);
    sum2_add(hi, lo, oh, ol);
    n += __shfl_down(n, off, 64);
  }
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) { sh[wave] = hi; sl[wave] = lo; si[wave] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    for (int w = 1; w < nw; ++w) {
      sum2_add(hi, lo, sh[w], sl[w]);
      n += si[w];
    }
  }
}

// part_loss holds (hi, lo) per block
__device__ __forceinline__ void write_partial(float hi, float lo, int cnt,
                                              float* part_loss, int* part_cnt) {
  block_sum2(hi, lo, cnt);
  if (threadIdx.x == 0) {
    part_loss[2 * blockIdx.x] = hi;
    part_loss[2 * blockIdx.x + 1] = lo;
    part_cnt[blockIdx.x] = cnt;
  }
}

__global__ void xent_finalize_kernel(const float* __restrict__ part_loss,
                                     const int* __restrict__ part_cnt, int nb,
                                     int mean, float* __restrict__ out_loss,
                                     int* __restrict__ out_cnt) {
  float hi = 0.f, lo = 0.f;
  int n = 0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    sum2_add(hi, lo, part_loss[2 * i], part_loss[2 * i + 1]);
    n += part_cnt[i];
  }
  block_sum2(hi, lo, n);
  if (threadIdx.x == 0) {
    float v = hi + lo;
    if (mean) {
      // one Newton step on the quotient: the division rounds once too
      float d = (float)(n > 1 ? n : 1);
      float q = v / d;
      float r = fmaf(-q, d, hi) + lo;
      v = q + r / d;
    }
    out_loss[0] = v;
    out_cnt[0] = n;
  }
}

// ---------------------------------------------------------------------------
// rows: one 256-thread block per row (C >= 64)
// ---------------------------------------------------------------------------

template <typename T>
__global__ void xent_rows_fwd_kernel(const T* __restrict__ logits,
                                     const long* __restrict__ target,
                                     float* __restrict__ loss,
                                     float* __restrict__ lse,
                                     float* __restrict__ part_loss,
                                     int* __restrict__ part_cnt, long P,
                                     XentArgs a) {
  __shared__ float scratch[8];
  const int C = a.C;
  float acc = 0.f, acc_lo = 0.f;
  int cnt = 0;
  for (long n = blockIdx.x; n < P; n += gridDim.x) {
    const T* row = logits + n * C;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += blockDim.x)
      m = fmaxf(m, (float)row[c]);
    m = block_max<256>(m, scratch);
    if (threadIdx.x == 0) scratch[0] = m;
    __syncthreads();
    m = scratch[0];
    __syncthreads();
    float s = 0.f, sx = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      float x = (float)row[c];
      s += __expf(x - m);
      sx += x;
    }
    s = block_sum<256>(s, scratch);
    __syncthreads();
    sx = block_sum<256>(sx, scratch);
    if (threadIdx.x == 0) {
      float l = m + __logf(s);
      lse[n] = l;
      long t = target[n];
      float v = 0.f;
      if (target_ok(t, a)) {
        v = row_loss(l, (float)row[t], sx, a);
        cnt += 1;
      }
      if (loss) loss[n] = v;
      sum2_add(acc, acc_lo, v, 0.f);
    }
    __syncthreads();
  }
  if (part_loss && threadIdx.x == 0) {
    part_loss[2 * blockIdx.x] = acc;
    part_loss[2 * blockIdx.x + 1] = acc_lo;
    part_cnt[blockIdx.x] = cnt;
  }
}

template <typename T>
__global__ void xent_rows_bwd_kernel(const T* __restrict__ logits,
                                     const float* __restrict__ lse,
                                     const long* __restrict__ target,
                                     XentGrad g, T* __restrict__ dlogits,
                                     long total, XentArgs a) {
  const float scale = grad_scale(g);
  const float hot = 1.f - a.eps;
  const float smooth = a.eps / (float)a.C;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    long n = idx / a.C;
    int c = (int)(idx - n * a.C);
    long t = target[n];
    float d = 0.f;
    if (target_ok(t, a)) {
      float gi = g.rows ? g.rows[n] : scale;
      float p = __expf((float)logits[idx] - lse[n]);
      d = (p - (t == c ? hot : 0.f) - smooth) * gi;
    }
    dlogits[idx] = (T)d;
  }
}

// ---------------------------------------------------------------------------
// strided: standard-contiguous (N, C, S); a lane owns V consecutive pixels
// ---------------------------------------------------------------------------

template <typename T, int V>
__device__ __forceinline__ void load_px(const T* p, float* out) {
  if constexpr (V == 1) out[0] = (float)p[0];
  else XVec<T>::load(p, out);
}

template <typename T, int V>
__device__ __forceinline__ void store_px(T* p, const float* in) {
  if constexpr (V == 1) p[0] = (T)in[0];
  else XVec<T>::store(p, in);
}

// P = N*S pixels in groups of V; S % V == 0 so a group never straddles images
template <typename T, int V>
__global__ void xent_strided_fwd_kernel(const T* __restrict__ logits,
                                        const long* __restrict__ target,
                                        float* __restrict__ loss,
                                        float* __restrict__ lse,
                                        float* __restrict__ part_loss,
                                        int* __restrict__ part_cnt, long P,
                                        long S, XentArgs a) {
  const int C = a.C;
  const long groups = P / V;
  float acc = 0.f, acc_lo = 0.f;
  int cnt = 0;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups;
       gi += (long)gridDim.x * blockDim.x) {
    const long p0 = gi * V;
    const long n = p0 / S;
    const T* base = logits + n * C * S + (p0 - n * S);
    int t[V];   // -1 marks an ignored pixel
    float m[V], s[V], sx[V], xt[V];
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      long tj = target[p0 + j];
      t[j] = target_ok(tj, a) ? (int)tj : -1;
    }
    load_px<T, V>(base, m);
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      s[j] = 1.f;
      sx[j] = m[j];
      xt[j] = m[j];   // class 0; overwritten when the target is another class
    }
    for (int c = 1; c < C; ++c) {
      float x[V];
      load_px<T, V>(base + (long)c * S, x);
      #pragma unroll
      for (int j = 0; j < V; ++j) {
        if (x[j] > m[j]) {
          s[j] = s[j] * expf(m[j] - x[j]) + 1.f;
          m[j] = x[j];
        } else if (x[j] != -INFINITY) {
          s[j] += expf(x[j] - m[j]);
        }
        sx[j] += x[j];
        if (t[j] == c) xt[j] = x[j];
      }
    }
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      float l = m[j] + logf(s[j]);
      lse[p0 + j] = l;
      float v = 0.f;
      if (t[j] >= 0) {
        v = row_loss(l, xt[j], sx[j], a);
        cnt += 1;
      }
      if (loss) loss[p0 + j] = v;
      sum2_add(acc, acc_lo, v, 0.f);
    }
  }
  if (part_loss) write_partial(acc, acc_lo, cnt, part_loss, part_cnt);
}

template <typename T, int V>
__global__ void xent_strided_bwd_kernel(const T* __restrict__ logits,
                                        const float* __restrict__ lse,
                                        const long* __restrict__ target,
                                        XentGrad g, T* __restrict__ dlogits,
                                        long P, long S, XentArgs a) {
  const int C = a.C;
  const long groups = P / V;
  const float scale = grad_scale(g);
  const float hot = 1.f - a.eps;
  const float smooth = a.eps / (float)C;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups;
       gi += (long)gridDim.x * blockDim.x) {
    const long p0 = gi * V;
    const long n = p0 / S;
    const long off = n * C * S + (p0 - n * S);
    int t[V];   // -1 marks an ignored pixel: its gradient is written as +0
    float l[V], gr[V];
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      long tj = target[p0 + j];
      t[j] = target_ok(tj, a) ? (int)tj : -1;
      l[j] = lse[p0 + j];
      gr[j] = g.rows ? g.rows[p0 + j] : scale;
    }
    for (int c = 0; c < C; ++c) {
      float x[V], d[V];
      load_px<T, V>(logits + off + (long)c * S, x);
      #pragma unroll
      for (int j = 0; j < V; ++j) {
        float p = expf(x[j] - l[j]);
        d[j] = t[j] < 0 ? 0.f
                        : (p - (t[j] == c ? hot : 0.f) - smooth) * gr[j];
      }
      store_px<T, V>(dlogits + off + (long)c * S, d);
    }
  }
}

// ---------------------------------------------------------------------------
// tile: R class-contiguous rows through LDS (C < 64); blockDim.x == R
// ---------------------------------------------------------------------------

// Copy `nelem` contiguous elements starting at `src` (16 B aligned when vec
// is set) into the fp32 tile: element e lands at tile[(e / C) * LS + e % C].
template <typename T>
__device__ __forceinline__ void tile_load(const T* __restrict__ src, int nelem,
                                          float* tile, int C, int LS, bool vec) {
  constexpr int V = XVec<T>::V;
  const int nvec = vec ? nelem / V : 0;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    float x[V];
    XVec<T>::load(src + (long)i * V, x);
    int e = i * V;
    int r = e / C;
    int c = e - r * C;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      tile[r * LS + c] = x[j];
      if (++c == C) { c = 0; ++r; }
    }
  }
  for (int e = nvec * V + threadIdx.x; e < nelem; e += blockDim.x) {
    int r = e / C;
    tile[r * LS + (e - r * C)] = (float)src[e];
  }
}

template <typename T>
__device__ __forceinline__ void tile_store(T* __restrict__ dst, int nelem,
                                           const float* tile, int C, int LS,
                                           bool vec) {
  constexpr int V = XVec<T>::V;
  const int nvec = vec ? nelem / V : 0;
  for (int i = threadIdx.x; i < nvec; i += blockDim.x) {
    float x[V];
    int e = i * V;
    int r = e / C;
    int c = e - r * C;
    #pragma unroll
    for (int j = 0; j < V; ++j) {
      x[j] = tile[r * LS + c];
      if (++c == C) { c = 0; ++r; }
    }
    XVec<T>::store(dst + (long)i * V, x);
  }
  for (int e = nvec * V + threadIdx.x; e < nelem; e += blockDim.x) {
    int r = e / C;
    dst[e] = (T)tile[r * LS + (e - r * C)];
  }
}

template <typename T>
__global__ void xent_tile_fwd_kernel(const T* __restrict__ logits,
                                     const long* __restrict__ target,
                                     float* __restrict__ loss,
                                     float* __restrict__ lse,
                                     float* __restrict__ part_loss,
                                     int* __restrict__ part_cnt, long P,
                                     int vec, XentArgs a) {
  extern __shared__ float tile[];
  const int C = a.C;
  const int LS = C | 1;
  const int R = blockDim.x;
  const long ntiles = (P + R - 1) / R;
  float acc = 0.f, acc_lo = 0.f;
  int cnt = 0;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long row0 = tl * R;
    const int rows = (int)((P - row0) < (long)R ? (P - row0) : (long)R);
    tile_load<T>(logits + row0 * C, rows * C, tile, C, LS, vec != 0);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      const float* x = tile + threadIdx.x * LS;
      const long row = row0 + threadIdx.x;
      float m = x[0];
      for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
      float s = 0.f, sx = 0.f;
      for (int c = 0; c < C; ++c) {
        s += expf(x[c] - m);
        sx += x[c];
      }
      float l = m + logf(s);
      lse[row] = l;
      long t = target[row];
      float v = 0.f;
      if (target_ok(t, a)) {
        v = row_loss(l, x[(int)t], sx, a);
        cnt += 1;
      }
      if (loss) loss[row] = v;
      sum2_add(acc, acc_lo, v, 0.f);
    }
    __syncthreads();
  }
  if (part_loss) write_partial(acc, acc_lo, cnt, part_loss, part_cnt);
}

template <typename T>
__global__ void xent_tile_bwd_kernel(const T* __restrict__ logits,
                                     const float* __restrict__ lse,
                                     const long* __restrict__ target,
                                     XentGrad g, T* __restrict__ dlogits,
                                     long P, int vec, XentArgs a) {
  extern __shared__ float tile[];
  const int C = a.C;
  const int LS = C | 1;
  const int R = blockDim.x;
  const long ntiles = (P + R - 1) / R;
  const float scale = grad_scale(g);
  const float hot = 1.f - a.eps;
  const float smooth = a.eps / (float)C;
  for (long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const long row0 = tl * R;
    const int rows = (int)((P - row0) < (long)R ? (P - row0) : (long)R);
    tile_load<T>(logits + row0 * C, rows * C, tile, C, LS, vec != 0);
    __syncthreads();
    if ((int)threadIdx.x < rows) {
      float* x = tile + threadIdx.x * LS;
      const long row = row0 + threadIdx.x;
      const long t = target[row];
      if (target_ok(t, a)) {
        const float l = lse[row];
        const float gi = g.rows ? g.rows[row] : scale;
        for (int c = 0; c < C; ++c)
          x[c] = (expf(x[c] - l) - ((int)t == c ? hot : 0.f) - smooth) * gi;
      } else {
        for (int c = 0; c < C; ++c) x[c] = 0.f;
      }
    }
    __syncthreads();
    tile_store<T>(dlogits + row0 * C, rows * C, tile, C, LS, vec != 0);
    __syncthreads();
  }
}

int capped_grid(long want, int max_grid) {
  int cap = (max_grid > 0 && max_grid < TFOSR_MAX_GRID) ? max_grid
                                                        : TFOSR_MAX_GRID;
  return (int)(want < cap ? (want > 0 ? want : 1) : cap);
}

// rows per tile: keeps the fp32 tile at or below 16 KB so that several
// blocks share a CU's LDS
int tile_rows(int C) { return C <= 15 ? 256 : (C <= 31 ? 128 : 64); }

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

enum { XENT_ROWS = 0, XENT_STRIDED = 1, XENT_TILE = 2 };

// Number of blocks the forward of `family` launches: the length of the
// partials workspace the caller allocates for a reduced forward.
int tfosr_xent_dense_grid(int family, int is_bf16, long P, long S, int C,
                          int max_grid) {
  if (family == XENT_ROWS) return capped_grid(P, max_grid);
  if (family == XENT_TILE) {
    int R = tile_rows(C);
    return capped_grid((P + R - 1) / R, max_grid);
  }
  int V = is_bf16 ? 8 : 4;
  long groups = (S % V == 0) ? P / V : P;
  return capped_grid((groups + 255) / 256, max_grid);
}

// loss: per-row output (reduction none) or nullptr; part_loss (two floats
// per block) and part_cnt (one int per block): reduced forms, or nullptr.
void tfosr_xent_dense_fwd(int family, const void* logits, const long* target,
                          float* loss, float* lse, float* part_loss,
                          int* part_cnt, int is_bf16, long P, long S, int C,
                          long ignore_index, float eps, int max_grid,
                          hipStream_t st) {
  if (P <= 0) return;
  XentArgs a{ignore_index, eps, C};
  int grid = tfosr_xent_dense_grid(family, is_bf16, P, S, C, max_grid);
  if (family == XENT_ROWS) {
    if (is_bf16)
      hipLaunchKernelGGL(xent_rows_fwd_kernel<bf16_t>, dim3(grid), dim3(256),
                         0, st, (const bf16_t*)logits, target, loss, lse,
                         part_loss, part_cnt, P, a);
    else
      hipLaunchKernelGGL(xent_rows_fwd_kernel<float>, dim3(grid), dim3(256), 0,
                         st, (const float*)logits, target, loss, lse,
                         part_loss, part_cnt, P, a);
  } else if (family == XENT_TILE) {
    int R = tile_rows(C);
    size_t lds = (size_t)R * (C | 1) * sizeof(float);
    int vec = aligned16(logits);
    if (is_bf16)
      hipLaunchKernelGGL(xent_tile_fwd_kernel<bf16_t>, dim3(grid), dim3(R), lds,
                         st, (const bf16_t*)logits, target, loss, lse,
                         part_loss, part_cnt, P, vec, a);
    else
      hipLaunchKernelGGL(xent_tile_fwd_kernel<float>, dim3(grid), dim3(R), lds,
                         st, (const float*)logits, target, loss, lse,
                         part_loss, part_cnt, P, vec, a);
  } else {
    int V = is_bf16 ? 8 : 4;
    bool vec = S % V == 0 && aligned16(logits);
    // an unaligned base takes the scalar kernel on the same grid: the
    // grid-stride loop covers the rest, and the partials keep their length
    if (is_bf16 && vec)
      hipLaunchKernelGGL((xent_strided_fwd_kernel<bf16_t, 8>), dim3(grid),
                         dim3(256), 0, st, (const bf16_t*)logits, target, loss,
                         lse, part_loss, part_cnt, P, S, a);
    else if (is_bf16)
      hipLaunchKernelGGL((xent_strided_fwd_kernel<bf16_t, 1>), dim3(grid),
                         dim3(256), 0, st, (const bf16_t*)logits, target, loss,
                         lse, part_loss, part_cnt, P, S, a);
    else if (vec)
      hipLaunchKernelGGL((xent_strided_fwd_kernel<float, 4>), dim3(grid),
                         dim3(256), 0, st, (const float*)logits, target, loss,
                         lse, part_loss, part_cnt, P, S, a);
    else
      hipLaunchKernelGGL((xent_strided_fwd_kernel<float, 1>), dim3(grid),
                         dim3(256), 0, st, (const float*)logits, target, loss,
                         lse, part_loss, part_cnt, P, S, a);
  }
}

void tfosr_xent_dense_finalize(const float* part_loss, const int* part_cnt,
                               int nb, int mean, float* out_loss, int* out_cnt,
                               hipStream_t st) {
  hipLaunchKernelGGL(xent_finalize_kernel, dim3(1), dim3(256), 0, st,
                     part_loss, part_cnt, nb, mean, out_loss, out_cnt);
}

// Upstream gradient: grows (per row) for reduction none; otherwise gscalar
// (one float) with nvalid (one int) and mean = 1 for the mean reduction.
void tfosr_xent_dense_bwd(int family, const void* logits, const float* lse,
                          const long* target, const float* grows,
                          const float* gscalar, const int* nvalid, int mean,
                          void* dlogits, int is_bf16, long P, long S, int C,
                          long ignore_index, float eps, int max_grid,
                          hipStream_t st) {
  if (P <= 0) return;
  XentArgs a{ignore_index, eps, C};
  XentGrad g{grows, gscalar, nvalid, mean};
  if (family == XENT_ROWS) {
    long total = P * C;
    int grid = capped_grid((total + 255) / 256, max_grid);
    if (is_bf16)
      hipLaunchKernelGGL(xent_rows_bwd_kernel<bf16_t>, dim3(grid), dim3(256),
                         0, st, (const bf16_t*)logits, lse, target, g,
                         (bf16_t*)dlogits, total, a);
    else
      hipLaunchKernelGGL(xent_rows_bwd_kernel<float>, dim3(grid), dim3(256), 0,
                         st, (const float*)logits, lse, target, g,
                         (float*)dlogits, total, a);
  } else if (family == XENT_TILE) {
    int R = tile_rows(C);
    int grid = capped_grid((P + R - 1) / R, max_grid);
    size_t lds = (size_t)R * (C | 1) * sizeof(float);
    int vec = aligned16(logits) && aligned16(dlogits);
    if (is_bf16)
      hipLaunchKernelGGL(xent_tile_bwd_kernel<bf16_t>, dim3(grid), dim3(R), lds,
                         st, (const bf16_t*)logits, lse, target, g,
                         (bf16_t*)dlogits, P, vec, a);
    else
      hipLaunchKernelGGL(xent_tile_bwd_kernel<float>, dim3(grid), dim3(R), lds,
                         st, (const float*)logits, lse, target, g,
                         (float*)dlogits, P, vec, a);
  } else {
    int V = is_bf16 ? 8 : 4;
    bool vec = S % V == 0 && aligned16(logits) && aligned16(dlogits);
    long groups = vec ? P / V : P;
    int grid = capped_grid((groups + 255) / 256, max_grid);
    if (is_bf16 && vec)
      hipLaunchKernelGGL((xent_strided_bwd_kernel<bf16_t, 8>), dim3(grid),
                         dim3(256), 0, st, (const bf16_t*)logits, lse, target,
                         g, (bf16_t*)dlogits, P, S, a);
    else if (is_bf16)
      hipLaunchKernelGGL((xent_strided_bwd_kernel<bf16_t, 1>), dim3(grid),
                         dim3(256), 0, st, (const bf16_t*)logits, lse, target,
                         g, (bf16_t*)dlogits, P, S, a);
    else if (vec)
      hipLaunchKernelGGL((xent_strided_bwd_kernel<float, 4>), dim3(grid),
                         dim3(256), 0, st, (const float*)logits, lse, target,
                         g, (float*)dlogits, P, S, a);
    else
      hipLaunchKernelGGL((xent_strided_bwd_kernel<float, 1>), dim3(grid),
                         dim3(256), 0, st, (const float*)logits, lse, target,
                         g, (float*)dlogits, P, S, a);
  }
}

}  // extern "C"
