// Weight gradient of ConvTranspose2d k4 s2 p1 (output_padding 0) for gfx950.
//
//   dW[ci][co][r][s] = sum_{n,ih,iw} x[n,ih,iw,ci] * dy[n,2ih-1+r,2iw-1+s,co]
//
// with dy = 0 outside the image; x [N,Cin,H,W] and dy [N,Cout,2H,2W] are
// channels_last bf16 (a pixel stride above C is allowed: a channel slice of a
// wider tensor), dW is fp32 in the parameter's own [Cin,Cout,4,4] layout.
//
// Parity classes. A dy pixel of parity (ph, pw) = (oh & 1, ow & 1) meets the
// 2x2 taps r = 2a+1-ph, s = 2b+1-pw (a, b in {0, 1}) and no others. In the
// class's own coordinates (oh = 2j+ph, ow = 2i+pw) tap (a, b) pairs input
// pixel (ih, iw) with class pixel (ih+a-ph, iw+b-pw): a 2x2 stride-1 weight
// gradient against a pixel-stride-2 view of dy. A workgroup owns (slab of
// input rows, class, 64 ci, 64 co): 4 taps x 64 x 64 fp32 = 64 accumulator
// registers per thread at 256 threads; wave w holds the 32 ci of half (w & 1)
// and the 32 co of half (w >> 1), so 2 x-fragments and 8 dy-fragments feed
// 16 MFMAs (16x16x32 bf16, contraction over pixels) per 32-pixel K step.
//
// Staging. Input rows are numbered g = n*H + ih across the batch, which makes
// x one contiguous run of pixels and a class's dy row of g the dy row 2g+ph.
// A slab is walked in blocks of rb rows. Per block the workgroup stages, with
// 16 B chunks through registers (channels are the fast axis):
//   x    rb rows x W pixels x 64 ci
//   dy   rb+1 class rows (the block's rows and the one halo row the class
//        needs: above for ph = 1, below for ph = 0) x W pixels x 64 co
// once, each pixel 128 B of channels in a 144 B slot (the 16 B pad spreads
// the transposed reads over the banks), plus one all-zero pixel. All four
// taps read the same dy patch: tap (a, b) of pixel slot p is slot
// p + a*W + b - pw. Chunks of channels past Cin / Cout are staged as zeros
// and never loaded, rows outside [0, N*H) likewise.
//
// Fragments. Both operands are pixel-major, so the MFMA operands are
// transposed views, read with ds_read_b64_tr_b16 (semantics as measured in
// conv_wrw2.hip / tools/trprobe.hip): lane l supplies the address of pixel
// (l>>4)*8 + 4t + ((l&15)>>2), channel group l&3 of a 16-channel block, and
// receives channel l&15 of pixels (l>>4)*8 + 4t + 0..3. Since every lane
// brings its own address, the stride-2 gather costs nothing, the column halo
// needs no staging, and a tap that leaves the image (or a pixel past the
// block's end, or across an image boundary inside the block) is the same
// read pointed at the zero pixel: no branches in the K loop.
//
// Split over pixels. With one slab the workgroup stores dW directly. With
// more, it stores its partial as float4 (the 4 taps) into
// ws[slab][class][ci][co], and convt_wrw_reduce_kernel sums the slabs in
// index order and scatters the taps to [ci][co][r][s]: no atomics, the same
// bits every run. (wrw_reduce_kernel of conv_wrw2.hip sums columns in place;
// it cannot do the class -> tap permutation, and storing partials in the
// final layout would make every partial store a 4 B scatter.)
#include "tfosr_common.h"

typedef short ctw_s16x4 __attribute__((ext_vector_type(4)));
typedef short ctw_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ctw_f32x4 __attribute__((ext_vector_type(4)));
typedef int ctw_i32x4 __attribute__((ext_vector_type(4)));

#define CTW_AS3 __attribute__((address_space(3)))

constexpr int CTW_THREADS = 256;
constexpr int CTW_TILE = 64;           // channels per tile, both axes
constexpr int CTW_SLOT = 144;          // bytes per staged pixel (128 + pad)
constexpr int CTW_KSTEP = 32;          // pixels per MFMA
constexpr int CTW_LDS_SMALL = 64 * 1024;   // two workgroups per CU
constexpr int CTW_LDS_LARGE = 160 * 1024;  // wide images: one per CU
constexpr int CTW_TARGET_WGS = 1024;   // 2 resident per CU x 256 CUs x 2
constexpr int CTW_MIN_SLAB_PIX = 64;   // two K steps
constexpr long CTW_WS_CAP = 32L << 20;

// t = q*d + r for 0 <= t < 2^20, inv = 1.0f / d. The product is within
// t/d * 2^-22 of the quotient and the quotient of t + 0.5 is at least 0.5/d
// from an integer, so q is exact; the two fix-ups cost two instructions and
// make that a matter of proof, not of need.
__device__ __forceinline__ void ctw_divmod(int t, int d, float inv, int& q,
                                           int& r) {
  q = (int)(((float)t + 0.5f) * inv);
  r = t - q * d;
  if (r < 0) { r += d; --q; }
  if (r >= d) { r -= d; ++q; }
}

__global__ __launch_bounds__(CTW_THREADS, 2) void convt_wrw_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
    float* __restrict__ out, int direct, int H, int W, int Cin, int Cout,
    long xps, long dps, int G, int R, int rb, int nti, int nto) {
  extern __shared__ __attribute__((aligned(16))) char ctw_lds[];
  CTW_AS3 char* lds = (CTW_AS3 char*)ctw_lds;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int b = blockIdx.x;
  const int cot = b % nto; b /= nto;
  const int cit = b % nti; b /= nti;
  const int cls = b & 3, slab = b >> 2;
  const int ph = cls >> 1, pw = cls & 1;
  const int ci0 = cit * CTW_TILE, co0 = cot * CTW_TILE;
  const int g0 = slab * R, g1 = min(G, g0 + R);

  const int XP = rb * W;                            // x slots; dy follows
  const int zoff = (XP + (rb + 1) * W) * CTW_SLOT;  // the zero pixel
  if (t < CTW_SLOT / 16)
    *(CTW_AS3 ctw_i32x4*)(lds + zoff + t * 16) = (ctw_i32x4){0, 0, 0, 0};

  const float invW = 1.0f / (float)W, invH = 1.0f / (float)H;
  const bool smallH = H < (1 << 19);   // else rb < H: at most one wrap

  // wave w: ci blocks 2*(w&1) + {0,1}, co blocks 2*(w>>1) + {0,1}
  const int cg = (lane & 3) * 8;                 // channel group, bytes
  const int xblk = (wave & 1) * 64 + cg;         // two 32 B blocks
  const int dblk = (wave >> 1) * 64 + cg;
  const int pl = (lane >> 4) * 8 + ((lane & 15) >> 2);

  ctw_f32x4 acc[4][2][2];
  #pragma unroll
  for (int tp = 0; tp < 4; ++tp)
    #pragma unroll
    for (int i = 0; i < 2; ++i)
      #pragma unroll
      for (int j = 0; j < 2; ++j) acc[tp][i][j] = {0.f, 0.f, 0.f, 0.f};

  auto tr8 = [&](int off0, int off1) -> ctw_bf16x8 {
    ctw_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (CTW_AS3 ctw_s16x4*)(lds + off0));
    ctw_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (CTW_AS3 ctw_s16x4*)(lds + off1));
    ctw_bf16x8 f;
    f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3];
    f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
    return f;
  };

  for (int gb = g0; gb < g1; gb += rb) {
    const int nr = min(rb, g1 - gb);
    const int npix = nr * W;

    // ---- stage x: npix pixels x 8 chunks, contiguous pixels in HBM
    const bf16_t* xsrc = x + (long)gb * W * xps + ci0;
    #pragma unroll 4
    for (int q = t; q < npix * 8; q += CTW_THREADS) {
      const int p = q >> 3, c8 = q & 7;
      ctw_i32x4 v = {0, 0, 0, 0};
      if (ci0 + c8 * 8 < Cin)
        v = *(const ctw_i32x4*)(xsrc + (long)p * xps + c8 * 8);
      *(CTW_AS3 ctw_i32x4*)(lds + p * CTW_SLOT + c8 * 16) = v;
    }
    // ---- stage dy: class rows gb-ph .. gb-ph+nr, pixels at stride 2
    #pragma unroll 4
    for (int q = t; q < (nr + 1) * W * 8; q += CTW_THREADS) {
      const int pp = q >> 3, c8 = q & 7;
      int lr, i;
      ctw_divmod(pp, W, invW, lr, i);
      const long row = (long)gb - ph + lr;         // class row n*H + j
      ctw_i32x4 v = {0, 0, 0, 0};
      if (co0 + c8 * 8 < Cout && row >= 0 && row < G)
        v = *(const ctw_i32x4*)(
            dy + ((2 * row + ph) * (2L * W) + 2 * i + pw) * dps + co0 +
            c8 * 8);
      *(CTW_AS3 ctw_i32x4*)(lds + (XP + pp) * CTW_SLOT + c8 * 16) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();

    const int ihb = gb % H;
    const int nks = (npix + CTW_KSTEP - 1) / CTW_KSTEP;
    for (int ks = 0; ks < nks; ++ks) {
      int xo[2], dof[4][2];
      #pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int p = ks * CTW_KSTEP + pl + 4 * tt;
        const bool live = p < npix;
        int rl, iw, ih, nwrap;
        ctw_divmod(live ? p : 0, W, invW, rl, iw);
        if (smallH) {
          ctw_divmod(ihb + rl, H, invH, nwrap, ih);
        } else {
          ih = ihb + rl;
          if (ih >= H) ih -= H;
        }
        const bool h0 = live && ih - ph >= 0, h1 = live && ih + 1 - ph < H;
        const bool w0 = iw - pw >= 0, w1 = iw + 1 - pw < W;
        const int base = (XP + p - pw) * CTW_SLOT;
        xo[tt] = live ? p * CTW_SLOT : zoff;
        dof[0][tt] = h0 && w0 ? base : zoff;
        dof[1][tt] = h0 && w1 ? base + CTW_SLOT : zoff;
        dof[2][tt] = h1 && w0 ? base + W * CTW_SLOT : zoff;
        dof[3][tt] = h1 && w1 ? base + (W + 1) * CTW_SLOT : zoff;
      }
      ctw_bf16x8 xf[2], df[4][2];
      #pragma unroll
      for (int i = 0; i < 2; ++i)
        xf[i] = tr8(xo[0] + xblk + i * 32, xo[1] + xblk + i * 32);
      #pragma unroll
      for (int tp = 0; tp < 4; ++tp)
        #pragma unroll
        for (int j = 0; j < 2; ++j)
          df[tp][j] = tr8(dof[tp][0] + dblk + j * 32,
                          dof[tp][1] + dblk + j * 32);
      #pragma unroll
      for (int tp = 0; tp < 4; ++tp)
        #pragma unroll
        for (int i = 0; i < 2; ++i)
          #pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[tp][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                xf[i], df[tp][j], acc[tp][i][j], 0, 0, 0);
    }
    // drain the transposed reads before the next block's staging overwrites
    // the slots (see conv_wrw2.hip)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // acc[tp][i][j][e]: ci = ci0 + ((wave&1)*2 + i)*16 + (lane>>4)*4 + e,
  //                   co = co0 + ((wave>>1)*2 + j)*16 + (lane&15)
  #pragma unroll
  for (int i = 0; i < 2; ++i)
    #pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int co = co0 + ((wave >> 1) * 2 + j) * 16 + (lane & 15);
      #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ci = ci0 + ((wave & 1) * 2 + i) * 16 + (lane >> 4) * 4 + e;
        if (ci >= Cin || co >= Cout) continue;
        const long pair = (long)ci * Cout + co;
        if (direct) {
          #pragma unroll
          for (int tp = 0; tp < 4; ++tp)
            out[pair * 16 + (2 * (tp >> 1) + 1 - ph) * 4 +
                (2 * (tp & 1) + 1 - pw)] = acc[tp][i][j][e];
        } else {
          const long col = ((long)(slab * 4 + cls) * Cin) * Cout + pair;
          *(ctw_f32x4*)(out + col * 4) =
              (ctw_f32x4){acc[0][i][j][e], acc[1][i][j][e], acc[2][i][j][e],
                          acc[3][i][j][e]};
        }
      }
    }
}

// ws [slabs][4 classes][Cin*Cout] float4 (the class's taps) -> dW
// [Cin*Cout][4][4]. One thread per (class, ci, co); slabs are added in index
// order, four loads in flight.
__global__ __launch_bounds__(256) void convt_wrw_reduce_kernel(
    const ctw_f32x4* __restrict__ ws, float* __restrict__ dW, long pairs,
    int slabs) {
  const long per = 4 * pairs;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= per) return;
  ctw_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < slabs; s += 4) {
    ctw_f32x4 v[4];
    #pragma unroll
    for (int u = 0; u < 4; ++u)
      v[u] = s + u < slabs ? ws[(long)(s + u) * per + idx]
                           : (ctw_f32x4){0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int u = 0; u < 4; ++u) acc += v[u];
  }
  const int cls = (int)(idx / pairs);
  const long pair = idx - cls * pairs;
  const int ph = cls >> 1, pw = cls & 1;
  #pragma unroll
  for (int tp = 0; tp < 4; ++tp)
    dW[pair * 16 + (2 * (tp >> 1) + 1 - ph) * 4 + (2 * (tp & 1) + 1 - pw)] =
        acc[tp];
}

extern "C" {

// How the gradient of N images of H x W input pixels is launched. Returns 0
// when the kernel cannot take the shape (a row block of one input row and
// its halo does not fit in LDS: W above 378), else 1 and
//   rb       input rows per staged block
//   rows     input rows (of all N*H) per slab
//   slabs    pixel splits; 1 = the kernel stores dW itself, no workspace
//   tiles    64 x 64 channel tiles
//   grid     workgroups = slabs * 4 classes * tiles
// The slab count is the smallest of: enough workgroups to fill the device
// twice over; a workspace that is written and read back in no more bytes
// than x and dy themselves, and at most 32 MB; 64 pixels per slab.
int tfosr_convt_wrw_plan(long N, int H, int W, int Cin, int Cout, int* rb,
                         int* rows, int* slabs, int* tiles, int* grid,
                         long* ws_bytes, int* lds_bytes) {
  const long G = N * H;
  long fit = (CTW_LDS_SMALL / CTW_SLOT - 1) / W;     // (2 rb + 1) <= fit
  if (fit < 5) fit = (CTW_LDS_LARGE / CTW_SLOT - 1) / W;
  if (fit < 3) return 0;
  long r = (fit - 1) / 2;
  const int nt = ((Cin + CTW_TILE - 1) / CTW_TILE) *
                 ((Cout + CTW_TILE - 1) / CTW_TILE);
  const long slab_bytes = 64L * Cin * Cout;          // 16 floats per pair
  const long in_bytes = 2 * G * W * ((long)Cin + 4L * Cout);
  long s = (in_bytes < CTW_WS_CAP ? in_bytes : CTW_WS_CAP) / slab_bytes;
  const long s_fill = (CTW_TARGET_WGS + 4 * nt - 1) / (4 * nt);
  const long s_pix = G * W / CTW_MIN_SLAB_PIX;
  if (s > s_fill) s = s_fill;
  if (s > s_pix) s = s_pix;
  if (s < 1) s = 1;
  long R = (G + s - 1) / s;
  if (R > r) R = (R + r - 1) / r * r;   // whole blocks but for the last slab
  else r = R;
  s = (G + R - 1) / R;
  *rb = (int)r;
  *rows = (int)R;
  *slabs = (int)s;
  *tiles = nt;
  *grid = (int)(s * 4 * nt);
  *ws_bytes = s > 1 ? s * slab_bytes : 0;
  *lds_bytes = (int)(((2 * r + 1) * W + 1) * CTW_SLOT);
  return 1;
}

// xps / dps: pixel strides of x and dy in elements. ws: ws_bytes of the plan
// (unused when it is 0).
hipError_t tfosr_convt_wrw(const void* x, const void* dy, float* ws, float* dW,
                           long N, int H, int W, int Cin, int Cout, long xps,
                           long dps, hipStream_t st) {
  int rb, rows, slabs, tiles, grid, lds;
  long wsb;
  if (!tfosr_convt_wrw_plan(N, H, W, Cin, Cout, &rb, &rows, &slabs, &tiles,
                            &grid, &wsb, &lds))
    return hipErrorInvalidValue;
  if (lds > 64 * 1024) {  // opt-in, per device: asked for every time
    hipError_t err = hipFuncSetAttribute(
        (const void*)convt_wrw_kernel,
        hipFuncAttributeMaxDynamicSharedMemorySize, CTW_LDS_LARGE);
    if (err != hipSuccess) return err;
  }
  const int nti = (Cin + CTW_TILE - 1) / CTW_TILE;
  const int nto = (Cout + CTW_TILE - 1) / CTW_TILE;
  const int direct = slabs == 1;
  hipLaunchKernelGGL(convt_wrw_kernel, dim3(grid), dim3(CTW_THREADS), lds, st,
                     (const bf16_t*)x, (const bf16_t*)dy, direct ? dW : ws,
                     direct, H, W, Cin, Cout, xps, dps, (int)(N * H), rows,
                     rb, nti, nto);
  if (!direct) {
    const long pairs = (long)Cin * Cout;
    hipLaunchKernelGGL(convt_wrw_reduce_kernel,
                       dim3((unsigned)((4 * pairs + 255) / 256)), dim3(256), 0,
                       st, (const ctw_f32x4*)ws, dW, pairs, slabs);
  }
  return hipGetLastError();
}

}  // extern "C"
