// Depthwise 3x3 convolution (groups == C, padding 1, stride 1 or 2, no bias)
// for gfx950: forward, backward-data and weight-gradient on channels_last
// bf16 (8 channels per lane) or fp32 (4 per lane) activations.
//
// A depthwise conv has no reuse across channels: 9 FMAs per element, nothing
// for MFMA. These are streaming kernels in the style of maxpool.hip and
// bn_relu.hip: 16 B per lane with the channel vector fastest, so consecutive
// lanes read consecutive 16 B and a wave of a narrow layer (C = 32) still
// covers whole cache lines across neighbouring pixels.
//
//   weight  the module's fp32 [C,1,3,3] parameter, read directly. With bf16
//           activations each weight is rounded to bf16 (nearest-even) on
//           load, the value autocast hands the library; fp32 uses it as is.
//   fwd     a thread produces a strip of DW_STRIP outputs along W for one
//           channel vector and reuses its column loads from registers. fp32
//           accumulation in the fixed tap order (ky, kx) row-major, one
//           rounding to the output dtype. Row overlap is left to L2.
//   dgrad   the same arithmetic as a gather over dy. Stride 1 is the forward
//           kernel with the filter flipped. Stride 2 handles a (even, odd)
//           pixel pair along W: the even pixel has one live column tap, the
//           odd one two, and the row parity (uniform along a row) selects
//           one or two live row taps. No scatter, no atomics, no zero fill.
//   wrw     two deterministic stages. Stage one: a thread keeps one channel
//           vector for its whole life (9*V fp32 accumulators in registers)
//           and walks its block's slab of output pixels; the threads of a
//           block that share a channel vector meet through LDS in index
//           order and the block writes one [9][C] partial. Stage two adds
//           the partials in index order. Same bits every run.
//
// Every global load is predicated on its own bounds.
#include "tfosr_common.h"

typedef unsigned int u32;

#define DW_BLOCK 256
#define DW_STRIP 4          // forward / stride-1 dgrad outputs per thread
#define DW_PAIR 2           // stride-2 dgrad pixels per thread
#define DW_WRW_CV_MAX 64    // channel vectors a wrw block covers at most
#define DW_WRW_MIN_PIX 4    // output pixels per wrw thread before splitting
#define DW_WRW_MAX_BLOCKS 1024
#define DW_FIN_OUT 32       // finalize: outputs per block ...
#define DW_FIN_LANES 8      // ... and partial slices per output

template <typename T, int V>
struct DwIO;

template <>
struct DwIO<bf16_t, 8> {
  static __device__ __forceinline__ void load(const bf16_t* p, float* out) {
    s8v v = *(const s8v*)p;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.s = v[j];
      out[j] = (float)u.b;
    }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float* a) {
    s8v v;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      union { short s; bf16_t b; } u;
      u.b = f2bf(a[j]);
      v[j] = u.s;
    }
    *(s8v*)p = v;
  }
  static __device__ __forceinline__ float weight(float w) {
    return bf2f(f2bf(w));
  }
};

template <>
struct DwIO<float, 4> {
  static __device__ __forceinline__ void load(const float* p, float* out) {
    f4v v = *(const f4v*)p;
    #pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = v[j];
  }
  static __device__ __forceinline__ void store(float* p, const float* a) {
    f4v v;
    #pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = a[j];
    *(f4v*)p = v;
  }
  static __device__ __forceinline__ float weight(float w) { return w; }
};

// wt[tap][j] for the V channels of vector cv: 9*V contiguous floats of the
// [C,1,3,3] weight. Scalar loads: the parameter may be a view into a flat
// DDP bucket at any 4-byte offset. A thread loads them once (see dw_grid).
template <typename T, int V>
__device__ __forceinline__ void dw_load_weight(const float* __restrict__ w,
                                               u32 cv, float (*wt)[V]) {
  const float* p = w + (size_t)cv * V * 9;
  #pragma unroll
  for (int j = 0; j < V; ++j) {
    #pragma unroll
    for (int t = 0; t < 9; ++t) wt[t][j] = DwIO<T, V>::weight(p[j * 9 + t]);
  }
}

// Forward (FLIP = false): out[n,ho,wo] = sum in[n, ho*S-1+ky, wo*S-1+kx] * w[ky,kx].
// Stride-1 dgrad (FLIP = true, S = 1): out[n,h,w] = sum in[n, h+1-ky, w+1-kx] * w[ky,kx].
// `in` is IH x IW, `out` is OH x OW. The work list is (n, oh, strip, cv) with
// cv fastest; the launcher keeps the grid stride a multiple of Cv when the
// loop runs more than once, so the weights stay in registers across passes.
template <typename T, int V, int S, bool FLIP>
__global__ __launch_bounds__(DW_BLOCK) void dwconv3x3_strip(
    const T* __restrict__ in, const float* __restrict__ w, T* __restrict__ out,
    int N, int C, int IH, int IW, int OH, int OW) {
  constexpr int L = DW_STRIP;
  constexpr int NCOL = (L - 1) * S + 3;
  const u32 Cv = C / V;
  const u32 WS = (OW + L - 1) / L;
  const u32 total = (u32)N * OH * WS * Cv;
  float wt[9][V];
  u32 wcv = 0xffffffffu;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (u32)gridDim.x * blockDim.x) {
    const u32 cv = i % Cv;
    u32 rest = i / Cv;
    const u32 ws = rest % WS;
    rest /= WS;
    const u32 oh = rest % OH;
    const u32 n = rest / OH;
    if (cv != wcv) {
      dw_load_weight<T, V>(w, cv, wt);
      wcv = cv;
    }
    float acc[L][V];
    #pragma unroll
    for (int l = 0; l < L; ++l) {
      #pragma unroll
      for (int j = 0; j < V; ++j) acc[l][j] = 0.f;
    }
    const int ow0 = (int)ws * L;
    const int iw0 = ow0 * S - 1;  // column jc of the strip reads in[.., iw0 + jc]
    #pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int ih = FLIP ? (int)oh + 1 - ky : (int)oh * S - 1 + ky;
      if (ih < 0 || ih >= IH) continue;
      const T* row = in + ((size_t)n * IH + ih) * IW * C + (size_t)cv * V;
      #pragma unroll
      for (int c = 0; c < NCOL; ++c) {
        // flipped: walk the columns right to left so every output still adds
        // its taps in kx order
        const int jc = FLIP ? NCOL - 1 - c : c;
        const int iw = iw0 + jc;
        float v[V];
        if (iw >= 0 && iw < IW) {
          DwIO<T, V>::load(row + (size_t)iw * C, v);
        } else {
          #pragma unroll
          for (int j = 0; j < V; ++j) v[j] = 0.f;
        }
        #pragma unroll
        for (int l = 0; l < L; ++l) {
          const int kx = FLIP ? l + 2 - jc : jc - l * S;
          if (kx < 0 || kx > 2) continue;
          #pragma unroll
          for (int j = 0; j < V; ++j)
            acc[l][j] = fmaf(v[j], wt[ky * 3 + kx][j], acc[l][j]);
        }
      }
    }
    T* po = out + (((size_t)n * OH + oh) * OW + ow0) * C + (size_t)cv * V;
    #pragma unroll
    for (int l = 0; l < L; ++l) {
      if (ow0 + l < OW) DwIO<T, V>::store(po + (size_t)l * C, acc[l]);
    }
  }
}

// Stride-2 dgrad: dx[n,h,w] = sum over taps with (h+1-ky) and (w+1-kx) even
// of dy[n, (h+1-ky)/2, (w+1-kx)/2] * w[ky,kx]. A thread owns the pixel pair
// (w0 = 2p, w0 + 1) of one row:
//   even w0:     kx = 1 reads dy column p
//   odd  w0+1:   kx = 0 reads column p + 1, kx = 2 reads column p
//   even h:      ky = 1 reads dy row h/2
//   odd  h:      ky = 0 reads row (h+1)/2, ky = 2 reads row (h-1)/2
template <typename T, int V>
__global__ __launch_bounds__(DW_BLOCK) void dwconv3x3_dgrad_s2(
    const T* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
    int N, int C, int H, int W, int OH, int OW) {
  const u32 Cv = C / V;
  const u32 WP = (W + DW_PAIR - 1) / DW_PAIR;
  const u32 total = (u32)N * H * WP * Cv;
  float wt[9][V];
  u32 wcv = 0xffffffffu;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (u32)gridDim.x * blockDim.x) {
    const u32 cv = i % Cv;
    u32 rest = i / Cv;
    const int p = (int)(rest % WP);
    rest /= WP;
    const int h = (int)(rest % H);
    const u32 n = rest / H;
    if (cv != wcv) {
      dw_load_weight<T, V>(w, cv, wt);
      wcv = cv;
    }
    float a0[V], a1[V];
    #pragma unroll
    for (int j = 0; j < V; ++j) { a0[j] = 0.f; a1[j] = 0.f; }
    const int w0 = 2 * p;
    const bool has_odd = w0 + 1 < W;
    const bool has_right = has_odd && p + 1 < OW;
    // one live row tap on even rows, two on odd rows, in ky order
    const bool odd_row = h & 1;
    const int nrow = odd_row ? 2 : 1;
    for (int r = 0; r < nrow; ++r) {
      const int ky = odd_row ? 2 * r : 1;
      const int oh = (h + 1 - ky) >> 1;
      if (oh >= OH) continue;  // odd last row of an even-height image
      const T* row = dy + (((size_t)n * OH + oh) * OW + p) * C + (size_t)cv * V;
      float va[V], vb[V];
      DwIO<T, V>::load(row, va);  // p < OW always: 2p <= W - 1
      if (has_right) {
        DwIO<T, V>::load(row + C, vb);
      } else {
        #pragma unroll
        for (int j = 0; j < V; ++j) vb[j] = 0.f;
      }
      // ky is 0, 1 or 2 at run time: pick the filter row without indexing
      // the register array dynamically
      #pragma unroll
      for (int j = 0; j < V; ++j) {
        const float k0 = ky == 0 ? wt[0][j] : (ky == 1 ? wt[3][j] : wt[6][j]);
        const float k1 = ky == 0 ? wt[1][j] : (ky == 1 ? wt[4][j] : wt[7][j]);
        const float k2 = ky == 0 ? wt[2][j] : (ky == 1 ? wt[5][j] : wt[8][j]);
        a0[j] = fmaf(va[j], k1, a0[j]);
        a1[j] = fmaf(vb[j], k0, a1[j]);
        a1[j] = fmaf(va[j], k2, a1[j]);
      }
    }
    T* po = dx + (((size_t)n * H + h) * W + w0) * C + (size_t)cv * V;
    DwIO<T, V>::store(po, a0);
    if (has_odd) DwIO<T, V>::store(po + C, a1);
  }
}

// wrw stage one. Block (bx, by): output pixels [bx*slab, min(M, (bx+1)*slab))
// of the flat (n, ho, wo) list, channel vectors [by*cvb, (by+1)*cvb). Thread
// t: channel slot t % cvb, pixel lane t / cvb; lanes >= P (cvb does not
// divide the block) and slots past Cv idle. part is [gridDim.x][9][C].
template <typename T, int V, int S>
__global__ __launch_bounds__(DW_BLOCK) void dwconv3x3_wrw_partial(
    const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
    int C, int H, int W, int OH, int OW, int cvb, int P, u32 M, u32 slab) {
  __shared__ float red[DW_BLOCK * V];
  const int cvl = threadIdx.x % cvb;
  const int p = threadIdx.x / cvb;
  const u32 Cv = C / V;
  const u32 cv = blockIdx.y * cvb + cvl;
  const bool live = p < P && cv < Cv;
  float acc[9][V];
  #pragma unroll
  for (int t = 0; t < 9; ++t) {
    #pragma unroll
    for (int j = 0; j < V; ++j) acc[t][j] = 0.f;
  }
  const u32 m0 = blockIdx.x * slab;
  const u32 m1 = (M - m0 < slab) ? M : m0 + slab;
  if (live) {
    for (u32 m = m0 + p; m < m1; m += P) {
      const int wo = (int)(m % OW);
      u32 rest = m / OW;
      const int ho = (int)(rest % OH);
      const u32 n = rest / OH;
      float g[V];
      DwIO<T, V>::load(dy + (size_t)m * C + (size_t)cv * V, g);
      #pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int ih = ho * S - 1 + ky;
        if (ih < 0 || ih >= H) continue;
        const T* row = x + ((size_t)n * H + ih) * W * C + (size_t)cv * V;
        #pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int iw = wo * S - 1 + kx;
          if (iw < 0 || iw >= W) continue;
          float v[V];
          DwIO<T, V>::load(row + (size_t)iw * C, v);
          #pragma unroll
          for (int j = 0; j < V; ++j)
            acc[ky * 3 + kx][j] = fmaf(g[j], v[j], acc[ky * 3 + kx][j]);
        }
      }
    }
  }
  // pixel lanes 1..P-1 hand their sums to lane 0 of the same channel slot,
  // one tap at a time; lane 0 adds them in lane order
  #pragma unroll
  for (int t = 0; t < 9; ++t) {
    if (live && p > 0) {
      #pragma unroll
      for (int j = 0; j < V; ++j) red[(p * cvb + cvl) * V + j] = acc[t][j];
    }
    __syncthreads();
    if (live && p == 0) {
      for (int q = 1; q < P; ++q) {
        #pragma unroll
        for (int j = 0; j < V; ++j) acc[t][j] += red[(q * cvb + cvl) * V + j];
      }
      float* po = part + ((size_t)blockIdx.x * 9 + t) * C + (size_t)cv * V;
      #pragma unroll
      for (int j = 0; j < V; ++j) po[j] = acc[t][j];
    }
    __syncthreads();
  }
}

// wrw stage two: dw[c][t] = sum_b part[b][t][c]. DW_FIN_LANES threads per
// output each add every DW_FIN_LANES-th partial in index order, then the
// first adds the lane sums in lane order.
__global__ __launch_bounds__(DW_FIN_OUT * DW_FIN_LANES) void dwconv3x3_wrw_finalize(
    const float* __restrict__ part, float* __restrict__ dw, int C, int nblk) {
  __shared__ float red[DW_FIN_LANES][DW_FIN_OUT];
  const int o = threadIdx.x % DW_FIN_OUT;
  const int r = threadIdx.x / DW_FIN_OUT;
  const u32 nout = 9u * C;
  const u32 idx = blockIdx.x * DW_FIN_OUT + o;  // t * C + c
  float s = 0.f;
  if (idx < nout) {
    for (int b = r; b < nblk; b += DW_FIN_LANES) s += part[(size_t)b * nout + idx];
  }
  red[r][o] = s;
  __syncthreads();
  if (r == 0 && idx < nout) {
    s = red[0][o];
    #pragma unroll
    for (int q = 1; q < DW_FIN_LANES; ++q) s += red[q][o];
    const u32 t = idx / C, c = idx % C;
    dw[(size_t)c * 9 + t] = s;
  }
}

static u32 dw_gcd(u32 a, u32 b) {
  while (b) { u32 t = a % b; a = b; b = t; }
  return a;
}

// Grid for a (.., cv)-fastest work list. When the grid-stride loop runs more
// than once, round the grid down so the stride is a multiple of Cv and a
// thread keeps its channel vector (and its weights) across passes.
static int dw_grid(long total, u32 Cv) {
  int g = tfosr_grid(total, DW_BLOCK);
  if ((long)g * DW_BLOCK < total) {
    const u32 q = Cv / dw_gcd(Cv, DW_BLOCK);
    if ((u32)g >= q) g -= g % q;
  }
  return g;
}

template <typename T, int V>
static void dw_launch_fwd(const void* x, const float* w, void* y, int N, int C,
                          int H, int W, int OH, int OW, int S, hipStream_t s) {
  const long total = (long)N * OH * ((OW + DW_STRIP - 1) / DW_STRIP) * (C / V);
  const int grid = dw_grid(total, C / V);
  if (S == 1)
    hipLaunchKernelGGL((dwconv3x3_strip<T, V, 1, false>), dim3(grid),
                       dim3(DW_BLOCK), 0, s, (const T*)x, w, (T*)y, N, C, H, W,
                       OH, OW);
  else
    hipLaunchKernelGGL((dwconv3x3_strip<T, V, 2, false>), dim3(grid),
                       dim3(DW_BLOCK), 0, s, (const T*)x, w, (T*)y, N, C, H, W,
                       OH, OW);
}

template <typename T, int V>
static void dw_launch_dgrad(const void* dy, const float* w, void* dx, int N,
                            int C, int H, int W, int OH, int OW, int S,
                            hipStream_t s) {
  if (S == 1) {
    const long total = (long)N * H * ((W + DW_STRIP - 1) / DW_STRIP) * (C / V);
    hipLaunchKernelGGL((dwconv3x3_strip<T, V, 1, true>),
                       dim3(dw_grid(total, C / V)), dim3(DW_BLOCK), 0, s,
                       (const T*)dy, w, (T*)dx, N, C, OH, OW, H, W);
  } else {
    const long total = (long)N * H * ((W + DW_PAIR - 1) / DW_PAIR) * (C / V);
    hipLaunchKernelGGL((dwconv3x3_dgrad_s2<T, V>), dim3(dw_grid(total, C / V)),
                       dim3(DW_BLOCK), 0, s, (const T*)dy, w, (T*)dx, N, C, H,
                       W, OH, OW);
  }
}

template <typename T, int V>
static void dw_launch_wrw(const void* dy, const void* x, float* part, int C,
                          int H, int W, int OH, int OW, int S, int cvb, int P,
                          int grid_y, int nblk, long M, long slab,
                          hipStream_t s) {
  if (S == 1)
    hipLaunchKernelGGL((dwconv3x3_wrw_partial<T, V, 1>), dim3(nblk, grid_y),
                       dim3(DW_BLOCK), 0, s, (const T*)dy, (const T*)x, part,
                       C, H, W, OH, OW, cvb, P, (u32)M, (u32)slab);
  else
    hipLaunchKernelGGL((dwconv3x3_wrw_partial<T, V, 2>), dim3(nblk, grid_y),
                       dim3(DW_BLOCK), 0, s, (const T*)dy, (const T*)x, part,
                       C, H, W, OH, OW, cvb, P, (u32)M, (u32)slab);
}

extern "C" {

// The constants a caller (and the tests) size work from.
void tfosr_dwconv3x3_info(int* block, int* max_grid, int* strip, int* pair,
                          int* wrw_min_pix, int* wrw_max_blocks,
                          int* fin_lanes) {
  *block = DW_BLOCK;
  *max_grid = TFOSR_MAX_GRID;
  *strip = DW_STRIP;
  *pair = DW_PAIR;
  *wrw_min_pix = DW_WRW_MIN_PIX;
  *wrw_max_blocks = DW_WRW_MAX_BLOCKS;
  *fin_lanes = DW_FIN_LANES;
}

// How stage one of wrw splits M output pixels x Cv channel vectors:
//   grid_y  channel chunks, at most DW_WRW_CV_MAX vectors each, evenly sized
//           (Cv = 72 gives 2 x 36, not 64 + 8), so a 960-channel layer with
//           a 4 x 4 map still spreads over the chip along the channel axis
//   P       pixel lanes per channel slot, DW_BLOCK / cvb (the rest idle)
//   nblk    pixel slabs: one per P * DW_WRW_MIN_PIX pixels, capped so the
//           whole grid stays near DW_WRW_MAX_BLOCKS; every slab is non-empty
void tfosr_dwconv3x3_wrw_plan(long M, int Cv, int* grid_y, int* cvb, int* P,
                              int* nblk, long* slab) {
  *grid_y = (Cv + DW_WRW_CV_MAX - 1) / DW_WRW_CV_MAX;
  *cvb = (Cv + *grid_y - 1) / *grid_y;
  *P = DW_BLOCK / *cvb;
  long per = (long)*P * DW_WRW_MIN_PIX;
  long want = (M + per - 1) / per;
  long cap = DW_WRW_MAX_BLOCKS / *grid_y;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  *slab = (M + want - 1) / want;
  *nblk = (int)((M + *slab - 1) / *slab);
}

void tfosr_dwconv3x3_fwd(const void* x, const float* w, void* y, int is_bf16,
                         int N, int C, int H, int W, int OH, int OW, int S,
                         hipStream_t s) {
  if (is_bf16)
    dw_launch_fwd<bf16_t, 8>(x, w, y, N, C, H, W, OH, OW, S, s);
  else
    dw_launch_fwd<float, 4>(x, w, y, N, C, H, W, OH, OW, S, s);
}

void tfosr_dwconv3x3_dgrad(const void* dy, const float* w, void* dx,
                           int is_bf16, int N, int C, int H, int W, int OH,
                           int OW, int S, hipStream_t s) {
  if (is_bf16)
    dw_launch_dgrad<bf16_t, 8>(dy, w, dx, N, C, H, W, OH, OW, S, s);
  else
    dw_launch_dgrad<float, 4>(dy, w, dx, N, C, H, W, OH, OW, S, s);
}

// part: [nblk][9][C] fp32 workspace from tfosr_dwconv3x3_wrw_plan.
void tfosr_dwconv3x3_wrw(const void* dy, const void* x, float* part, float* dw,
                         int is_bf16, int N, int C, int H, int W, int OH,
                         int OW, int S, hipStream_t s) {
  const int V = is_bf16 ? 8 : 4;
  const long M = (long)N * OH * OW;
  int grid_y, cvb, P, nblk;
  long slab;
  tfosr_dwconv3x3_wrw_plan(M, C / V, &grid_y, &cvb, &P, &nblk, &slab);
  if (is_bf16)
    dw_launch_wrw<bf16_t, 8>(dy, x, part, C, H, W, OH, OW, S, cvb, P, grid_y,
                             nblk, M, slab, s);
  else
    dw_launch_wrw<float, 4>(dy, x, part, C, H, W, OH, OW, S, cvb, P, grid_y,
                            nblk, M, slab, s);
  const int nout = 9 * C;
  hipLaunchKernelGGL(dwconv3x3_wrw_finalize,
                     dim3((nout + DW_FIN_OUT - 1) / DW_FIN_OUT),
                     dim3(DW_FIN_OUT * DW_FIN_LANES), 0, s, part, dw, C, nblk);
}

}  // extern "C"
