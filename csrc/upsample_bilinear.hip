// Bilinear resize of 4-D channels_last tensors on gfx950, bf16 or fp32,
// upscale (or identity) on both axes, C in [1, 2048]: forward and backward.
// Arithmetic is fp32; every output is rounded once into the tensor's dtype.
//
// Index rule (ATen's upsample_bilinear2d with an output size), per axis:
//
//   align_corners = false   scale = in / out            (one fp32 division)
//                           src   = max(scale * (dst + 0.5) - 0.5, 0)
//   align_corners = true    scale = (in - 1) / (out - 1), or 0 when out == 1
//                           src   = scale * dst
//   taps                    i0 = floor(src), i1 = i0 + (i0 < in - 1),
//                           l1 = src - i0,   l0 = 1 - l1
//
// At the high edge of an align_corners = false upscale both taps are the last
// pixel with l1 != 0; that is the rule, not an accident. The scale is
// computed once on the host and handed to the kernels, so forward, backward
// and the tile planner all see the same float.
//
//   fwd   write-bound. A workgroup owns UB_FH (8) output rows x UB_FW (32)
//         output columns of one image, all channels (or a chunk of Cc when
//         the patch would not fit UB_LDS bytes). It stages the input patch
//         the tile reads (its first i0 to its last i1 on each axis: at most
//         tile + 2 rows and columns, 3 x 4 pixels at x16) into LDS as fp32,
//         keeps the (i0, i1, l1) of its 32 columns and 8 rows in LDS, lerps
//         vertically into an LDS band [8][patch_w * Cc] and expands that
//         horizontally: an output row segment is one contiguous run of
//         tile_w * C elements that is only element-aligned (C = 21: 42-byte
//         pixels), so lanes walk it in 16 B chunks cut on the grid of the
//         address itself; whole chunks are one 16 B store, the ragged head
//         and tail element stores. An element finds its (pixel, channel)
//         from its offset in the run: one division per chunk, a counter
//         after that. With channel chunks the run is one pixel's Cc elements
//         and a row has tile_w of them. No byte is written twice, none
//         outside the tensor.
//   bwd   a gather: no atomics, one summation order, same bits every run. A
//         workgroup owns UB_BH x UB_BW (8 x 8) input pixels and Cc <= 32
//         channels: lane t owns column t / Cc, channel t % Cc and keeps the
//         eight rows' sums in registers. The dy rows and columns whose taps
//         touch the tile are found by bisection on the index rule itself
//         (i0 and i1 are monotone in dst), so what forward scatters is what
//         backward gathers whatever the rounding of src. UB_BR (4) dy rows
//         at a time are staged into LDS in the tensor's dtype with 16 B
//         loads on the address grid (element loads at the ragged ends),
//         beside the (i0, i1, l1) of the staged columns; a lane reduces the
//         columns that feed its pixel in column order, multiplies by the
//         row's vertical weight and adds into the one or two rows that dy
//         row feeds. A segment wider than the LDS budget (huge scales) is
//         taken in pieces of P columns, in order. dx is written once.
//         dy re-read at the DeepLab head (32 x 32 -> 512 x 512, x16): rows
//         (8 + 1) / 8, columns (8 + 1) / 8 of what the tile owns, less at
//         the image border: 1.27x in the interior, 1.20x over the image.
//         A 1 x 1 input is the same kernel: one tile per (image, chunk),
//         every dy pixel has weight one, the sum runs in row-major order;
//         the ASPP pool branch (32 x 256 x 1 x 1) still gives 256 workgroups.
//
// Every global access is predicated on its own bounds, LDS tap indices are
// clamped to the staged patch, grids are capped at TFOSR_MAX_GRID with a
// stride loop for the rest.
#include "tfosr_common.h"

#define UB_BLOCK 256
#define UB_FH 8        // fwd: output rows per tile
#define UB_FW 32       //      output columns per tile
#define UB_BH 8        // bwd: input rows per tile
#define UB_BW 8        //      input columns per tile
#define UB_BR 4        //      dy rows staged together
#define UB_LDS 40960   // dynamic LDS a workgroup may ask for, bytes
#define UB_MAX_C 2048

typedef unsigned int ub_u4 __attribute__((ext_vector_type(4)));

struct UbAxis {
  int in, out;
  float scale;
  int align;
};

__device__ __forceinline__ float ub_ld(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float ub_ld(const float* p) { return *p; }
__device__ __forceinline__ void ub_cvt(float v, bf16_t* o) { *o = f2bf(v); }
__device__ __forceinline__ void ub_cvt(float v, float* o) { *o = v; }

__device__ __forceinline__ void ub_taps(const UbAxis& ax, int dst, int& i0,
                                        int& i1, float& l1) {
  const float src = ax.align
      ? ax.scale * (float)dst
      : fmaxf(ax.scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  const int i = min((int)src, ax.in - 1);
  i0 = i;
  i1 = i + (i < ax.in - 1 ? 1 : 0);
  l1 = src - (float)i;
}

// smallest dst in [0, out) whose i1 >= a, or out
__device__ __forceinline__ int ub_first_i1_ge(const UbAxis& ax, int a) {
  int lo = 0, hi = ax.out;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    int i0, i1;
    float l1;
    ub_taps(ax, mid, i0, i1, l1);
    if (i1 >= a) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// largest dst in [0, out) whose i0 <= a, or -1
__device__ __forceinline__ int ub_last_i0_le(const UbAxis& ax, int a) {
  int lo = 0, hi = ax.out;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    int i0, i1;
    float l1;
    ub_taps(ax, mid, i0, i1, l1);
    if (i0 > a) hi = mid;
    else lo = mid + 1;
  }
  return lo - 1;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// phc x pwc: the patch LDS is laid out for (tfosr_upsample_bilinear_plan).
template <typename T>
__global__ __launch_bounds__(UB_BLOCK) void upsample_bilinear_fwd_kernel(
    const T* __restrict__ x, T* __restrict__ y, int C, UbAxis ay, UbAxis ax,
    int Cc, int phc, int pwc, long tiles) {
  constexpr int VEC = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char ub_smem[];
  __shared__ int cx0[UB_FW], cx1[UB_FW], ry0[UB_FH], ry1[UB_FH];
  __shared__ float cl1[UB_FW], rl1[UB_FH];
  float* patch = (float*)ub_smem;         // [phc][pwc][Cc]
  float* vbuf = patch + phc * pwc * Cc;   // [UB_FH][pwc][Cc]

  const int t = threadIdx.x;
  const int TY = (ay.out + UB_FH - 1) / UB_FH;
  const int TX = (ax.out + UB_FW - 1) / UB_FW;
  const int NCH = (C + Cc - 1) / Cc;

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int chunk = (int)(tile % NCH);
    long rest = tile / NCH;
    const int tx = (int)(rest % TX);
    rest /= TX;
    const int ty = (int)(rest % TY);
    const int n = (int)(rest / TY);
    const int oy0 = ty * UB_FH, ox0 = tx * UB_FW;
    const int th = min(UB_FH, ay.out - oy0), tw = min(UB_FW, ax.out - ox0);
    const int c0 = chunk * Cc, cc = min(Cc, C - c0);

    int row_lo, row_hi, col_lo, col_hi, unused;
    float lam;
    ub_taps(ay, oy0, row_lo, unused, lam);
    ub_taps(ay, oy0 + th - 1, unused, row_hi, lam);
    ub_taps(ax, ox0, col_lo, unused, lam);
    ub_taps(ax, ox0 + tw - 1, unused, col_hi, lam);
    const int ph = min(row_hi - row_lo + 1, phc);
    const int pw = min(col_hi - col_lo + 1, pwc);

    __syncthreads();  // the previous tile is done with the tables and vbuf
    if (t < tw) {
      int i0, i1;
      ub_taps(ax, ox0 + t, i0, i1, lam);
      cx0[t] = min(i0 - col_lo, pw - 1);
      cx1[t] = min(i1 - col_lo, pw - 1);
      cl1[t] = lam;
    } else if (t >= 64 && t < 64 + th) {
      int i0, i1;
      ub_taps(ay, oy0 + t - 64, i0, i1, lam);
      ry0[t - 64] = min(i0 - row_lo, ph - 1);
      ry1[t - 64] = min(i1 - row_lo, ph - 1);
      rl1[t - 64] = lam;
    }
    for (int q = t; q < ph * pw * cc; q += UB_BLOCK) {
      const int p = q / cc, ch = q - p * cc;
      const int pr = p / pw, pc = p - pr * pw;
      const size_t g =
          (((size_t)n * ay.in + row_lo + pr) * ax.in + col_lo + pc) * C + c0 + ch;
      patch[(pr * pwc + pc) * Cc + ch] = ub_ld(x + g);
    }
    __syncthreads();

    for (int q = t; q < th * pw * cc; q += UB_BLOCK) {
      const int p = q / cc, ch = q - p * cc;
      const int r = p / pw, pc = p - r * pw;
      const float l1 = rl1[r];
      const float a = patch[(ry0[r] * pwc + pc) * Cc + ch];
      const float b = patch[(ry1[r] * pwc + pc) * Cc + ch];
      vbuf[(r * pwc + pc) * Cc + ch] = (1.f - l1) * a + l1 * b;
    }
    __syncthreads();

    // runs of `runlen` contiguous output elements: the whole row segment, or
    // one pixel's chunk. Chunk c of a run covers elements
    // (g0 & ~(VEC - 1)) + c * VEC .. + VEC of y.
    const int ppr = NCH == 1 ? tw : 1, nruns = NCH == 1 ? 1 : tw;
    const int runlen = ppr * cc;
    const int CH = (runlen + VEC - 1) / VEC + 1;
    for (int q = t; q < th * nruns * CH; q += UB_BLOCK) {
      const int p = q / CH, c = q - p * CH;
      const int r = p / nruns, run = p - r * nruns;
      const size_t g0 =
          (((size_t)n * ay.out + oy0 + r) * ax.out + ox0 + run * ppr) * C + c0;
      const size_t k0 = (g0 & ~(size_t)(VEC - 1)) + (size_t)c * VEC;
      if (k0 >= g0 + runlen) continue;
      const int e0 = (int)((long)k0 - (long)g0);  // negative in the head
      const float* vrow = vbuf + r * pwc * Cc;
      const int first = max(e0, 0);
      int px = first / cc, ch = first - px * cc;
      px += run * ppr;
      union { ub_u4 v; T s[VEC]; } o;
      #pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int e = e0 + j;
        if (e >= 0 && e < runlen) {
          const float l1 = cl1[px];
          const float v = (1.f - l1) * vrow[cx0[px] * Cc + ch] +
                          l1 * vrow[cx1[px] * Cc + ch];
          ub_cvt(v, &o.s[j]);
          if (++ch == cc) {
            ch = 0;
            ++px;
          }
        }
      }
      if (e0 >= 0 && e0 + VEC <= runlen) {
        *(ub_u4*)(y + k0) = o.v;
      } else {
        #pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const int e = e0 + j;
          if (e >= 0 && e < runlen) y[k0 + j] = o.s[j];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

// P: columns of dy staged at a time (tfosr_upsample_bilinear_plan).
template <typename T>
__global__ __launch_bounds__(UB_BLOCK) void upsample_bilinear_bwd_kernel(
    const T* __restrict__ dy, T* __restrict__ dx, int C, UbAxis ay, UbAxis ax,
    int Cc, int P, long tiles) {
  constexpr int VEC = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char ub_smem[];
  __shared__ int sy0[UB_BR], sy1[UB_BR];
  __shared__ float sl1[UB_BR];
  int* ti0 = (int*)ub_smem;        // [P] taps of the staged columns
  int* ti1 = ti0 + P;
  float* tl1 = (float*)(ti1 + P);
  T* seg = (T*)(tl1 + P);          // [UB_BR][P][Cc]

  const int t = threadIdx.x;
  const int TY = (ay.in + UB_BH - 1) / UB_BH;
  const int TX = (ax.in + UB_BW - 1) / UB_BW;
  const int NCH = (C + Cc - 1) / Cc;
  const int ixl = t / Cc, ch = t - ixl * Cc;

  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int chunk = (int)(tile % NCH);
    long rest = tile / NCH;
    const int tx = (int)(rest % TX);
    rest /= TX;
    const int ty = (int)(rest % TY);
    const int n = (int)(rest / TY);
    const int a = ty * UB_BH, b = tx * UB_BW;
    const int th = min(UB_BH, ay.in - a), tw = min(UB_BW, ax.in - b);
    const int c0 = chunk * Cc, cc = min(Cc, C - c0);

    // dy rows and columns with a tap in the tile, then this lane's columns
    const int oy_lo = ub_first_i1_ge(ay, a);
    const int oy_hi = ub_last_i0_le(ay, a + th - 1);
    const int ox_lo = ub_first_i1_ge(ax, b);
    const int ox_hi = ub_last_i0_le(ax, b + tw - 1);
    const bool active = ixl < tw && ch < cc;
    const int ix = b + ixl;
    const int lx_lo = active ? ub_first_i1_ge(ax, ix) : 0;
    const int lx_hi = active ? ub_last_i0_le(ax, ix) : -1;

    float acc[UB_BH];
    #pragma unroll
    for (int k = 0; k < UB_BH; ++k) acc[k] = 0.f;

    for (int oyb = oy_lo; oyb <= oy_hi; oyb += UB_BR) {
      const int nr = min(UB_BR, oy_hi - oyb + 1);
      for (int px = ox_lo; px <= ox_hi; px += P) {
        const int pw = min(P, ox_hi - px + 1);
        __syncthreads();  // the previous piece has been reduced
        for (int q = t; q < pw; q += UB_BLOCK) {
          int i0, i1;
          float l1;
          ub_taps(ax, px + q, i0, i1, l1);
          ti0[q] = i0;
          ti1[q] = i1;
          tl1[q] = l1;
        }
        if (t < nr) {
          int i0, i1;
          float l1;
          ub_taps(ay, oyb + t, i0, i1, l1);
          sy0[t] = i0;
          sy1[t] = i1;
          sl1[t] = l1;
        }
        // runs as in the forward: the whole piece of a row, or one pixel's
        // chunk; element e of a run lands at seg[r][run * ppr * Cc + e]
        const int ppr = NCH == 1 ? pw : 1, nruns = NCH == 1 ? 1 : pw;
        const int runlen = ppr * cc;
        const int CH = (runlen + VEC - 1) / VEC + 1;
        for (int q = t; q < nr * nruns * CH; q += UB_BLOCK) {
          const int p = q / CH, c = q - p * CH;
          const int r = p / nruns, run = p - r * nruns;
          const size_t g0 =
              (((size_t)n * ay.out + oyb + r) * ax.out + px + run * ppr) * C + c0;
          const size_t k0 = (g0 & ~(size_t)(VEC - 1)) + (size_t)c * VEC;
          if (k0 >= g0 + runlen) continue;
          const int e0 = (int)((long)k0 - (long)g0);
          T* dst = seg + (r * P + run * ppr) * Cc;
          if (e0 >= 0 && e0 + VEC <= runlen) {
            union { ub_u4 v; T s[VEC]; } in;
            in.v = *(const ub_u4*)(dy + k0);
            #pragma unroll
            for (int j = 0; j < VEC; ++j) dst[e0 + j] = in.s[j];
          } else {
            #pragma unroll
            for (int j = 0; j < VEC; ++j) {
              const int e = e0 + j;
              if (e >= 0 && e < runlen) dst[e] = dy[k0 + j];
            }
          }
        }
        __syncthreads();
        if (active) {
          const int lo = max(lx_lo, px), hi = min(lx_hi, px + pw - 1);
          for (int r = 0; r < nr; ++r) {
            const T* srow = seg + r * P * Cc + ch;
            float h = 0.f;
            for (int ox = lo; ox <= hi; ++ox) {
              const int q = ox - px;
              const float l1 = tl1[q];
              const float w = (ti0[q] == ix ? 1.f - l1 : 0.f) +
                              (ti1[q] == ix ? l1 : 0.f);
              h += w * ub_ld(srow + q * Cc);
            }
            const int y0 = sy0[r], y1 = sy1[r];
            const float l1y = sl1[r];
            #pragma unroll
            for (int k = 0; k < UB_BH; ++k) {
              if (y0 == a + k || y1 == a + k) {
                const float wy = (y0 == a + k ? 1.f - l1y : 0.f) +
                                 (y1 == a + k ? l1y : 0.f);
                acc[k] += wy * h;
              }
            }
          }
        }
      }
    }
    if (active) {
      #pragma unroll
      for (int k = 0; k < UB_BH; ++k) {
        if (k < th)
          ub_cvt(acc[k],
                 dx + (((size_t)n * ay.in + a + k) * ax.in + ix) * C + c0 + ch);
      }
    }
  }
}

static float ub_scale(int in, int out, int align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}

// Rows (columns) of input a band of `tile` outputs can read: consecutive src
// differ by scale <= 1, so i0 spans floor((tile - 1) * scale) + 2 at most, i1
// adds one, and one more absorbs the rounding of src.
static int ub_patch_cap(int in, int tile, float scale) {
  int cap = (int)((float)(tile - 1) * scale) + 4;
  if (cap > tile + 2) cap = tile + 2;
  return cap < in ? cap : in;
}

extern "C" {

// The constants a caller (and the tests) size work from.
void tfosr_upsample_bilinear_info(int* block, int* max_grid, int* fwd_tile_h,
                                  int* fwd_tile_w, int* bwd_tile_h,
                                  int* bwd_tile_w, int* bwd_rows, int* lds,
                                  int* max_c) {
  *block = UB_BLOCK;
  *max_grid = TFOSR_MAX_GRID;
  *fwd_tile_h = UB_FH;
  *fwd_tile_w = UB_FW;
  *bwd_tile_h = UB_BH;
  *bwd_tile_w = UB_BW;
  *bwd_rows = UB_BR;
  *lds = UB_LDS;
  *max_c = UB_MAX_C;
}

// How a shape is split. fwd: channels per chunk and the patch the LDS is laid
// out for; bwd: channels per chunk (one lane per column and channel) and the
// dy columns staged at a time. tiles are per image.
void tfosr_upsample_bilinear_plan(int C, int Hin, int Win, int Hout, int Wout,
                                  int align, int itemsize, int* fwd_cc,
                                  int* fwd_ph, int* fwd_pw, long* fwd_tiles,
                                  int* bwd_cc, int* bwd_p, long* bwd_tiles) {
  const int ph = ub_patch_cap(Hin, UB_FH, ub_scale(Hin, Hout, align));
  const int pw = ub_patch_cap(Win, UB_FW, ub_scale(Win, Wout, align));
  int cc = UB_LDS / (4 * (ph + UB_FH) * pw);
  if (cc > C) cc = C;
  *fwd_cc = cc;
  *fwd_ph = ph;
  *fwd_pw = pw;
  *fwd_tiles = (long)((Hout + UB_FH - 1) / UB_FH) *
               ((Wout + UB_FW - 1) / UB_FW) * ((C + cc - 1) / cc);
  int bc = UB_BLOCK / UB_BW;
  if (bc > C) bc = C;
  long need = (long)(UB_BW + 1) * ((Wout + Win - 1) / Win) + 2;
  if (need > Wout) need = Wout;
  const long fit = UB_LDS / (12 + UB_BR * bc * itemsize);
  *bwd_cc = bc;
  *bwd_p = (int)(need < fit ? need : fit);
  *bwd_tiles = (long)((Hin + UB_BH - 1) / UB_BH) *
               ((Win + UB_BW - 1) / UB_BW) * ((C + bc - 1) / bc);
}

void tfosr_upsample_bilinear_fwd(const void* x, void* y, int bf16, int N,
                                 int C, int Hin, int Win, int Hout, int Wout,
                                 int align, hipStream_t s) {
  int fcc, ph, pw, bcc, bp;
  long ftiles, btiles;
  tfosr_upsample_bilinear_plan(C, Hin, Win, Hout, Wout, align, bf16 ? 2 : 4,
                               &fcc, &ph, &pw, &ftiles, &bcc, &bp, &btiles);
  const UbAxis ay = {Hin, Hout, ub_scale(Hin, Hout, align), align};
  const UbAxis ax = {Win, Wout, ub_scale(Win, Wout, align), align};
  const long tiles = ftiles * N;
  const int grid = tfosr_grid(tiles, 1);
  const size_t lds = (size_t)4 * (ph + UB_FH) * pw * fcc;
  if (bf16)
    hipLaunchKernelGGL((upsample_bilinear_fwd_kernel<bf16_t>), dim3(grid),
                       dim3(UB_BLOCK), lds, s, (const bf16_t*)x, (bf16_t*)y,
                       C, ay, ax, fcc, ph, pw, tiles);
  else
    hipLaunchKernelGGL((upsample_bilinear_fwd_kernel<float>), dim3(grid),
                       dim3(UB_BLOCK), lds, s, (const float*)x, (float*)y, C,
                       ay, ax, fcc, ph, pw, tiles);
}

void tfosr_upsample_bilinear_bwd(const void* dy, void* dx, int bf16, int N,
                                 int C, int Hin, int Win, int Hout, int Wout,
                                 int align, hipStream_t s) {
  int fcc, ph, pw, bcc, bp;
  long ftiles, btiles;
  const int itemsize = bf16 ? 2 : 4;
  tfosr_upsample_bilinear_plan(C, Hin, Win, Hout, Wout, align, itemsize, &fcc,
                               &ph, &pw, &ftiles, &bcc, &bp, &btiles);
  const UbAxis ay = {Hin, Hout, ub_scale(Hin, Hout, align), align};
  const UbAxis ax = {Win, Wout, ub_scale(Win, Wout, align), align};
  const long tiles = btiles * N;
  const int grid = tfosr_grid(tiles, 1);
  const size_t lds = (size_t)bp * (12 + UB_BR * bcc * itemsize);
  if (bf16)
    hipLaunchKernelGGL((upsample_bilinear_bwd_kernel<bf16_t>), dim3(grid),
                       dim3(UB_BLOCK), lds, s, (const bf16_t*)dy, (bf16_t*)dx,
                       C, ay, ax, bcc, bp, tiles);
  else
    hipLaunchKernelGGL((upsample_bilinear_bwd_kernel<float>), dim3(grid),
                       dim3(UB_BLOCK), lds, s, (const float*)dy, (float*)dx,
                       C, ay, ax, bcc, bp, tiles);
}

}  // extern "C"
