// Halo-staged 3x3 stride-1 padding-1 convolution for gfx950 (NHWC bf16):
//
//   out[M = N*H*W, Cout] = sum over 32-channel chunks c, taps (r, s) of
//       x[m + (r-1)*W + (s-1)][c] @ W9[Cout][r][s][c]^T
//
// conv3x3_mfma.hip walks K tap-major: every 32-wide K-step stages one tap of
// one channel chunk, so each pixel's 64 B chunk reaches LDS nine times, each
// time behind its own pair of barriers. This kernel walks K chunk-major. For
// a tile of BM consecutive output pixels (flattened (n, oh, ow) index) it
// stages, once per chunk,
//
//   span : pixels [m0 - (W+1), m0 + BM + (W+1)) of the chunk, 64 B each
//   slab : W9[tile_n .. +64][all 9 taps][chunk], 9 * 64 * 64 B = 36 KB
//
// and runs all nine taps from LDS between ONE pair of barriers: tap (r, s) of
// the tile's pixel i is span row i + r*W + s. The span is addressed by the
// flattened pixel index alone, clamped into the tensor, with full EXEC; what
// a tap may not see (rows and columns outside the pixel's own image, which in
// the span are a neighbouring row, a neighbouring image or a clamped pixel)
// is removed at fragment level: every lane knows a 9-bit tap mask for each of
// its fragment pixels and zeroes the A fragment after the LDS read. No zero
// guard buffer is involved.
//
// Overlap comes from occupancy, not from a ring: the buffer is single (span +
// slab <= 80 KB) so that two workgroups are resident per CU; while one waits
// for its chunk the other multiplies.
//
// LDS image: 64 B rows, 16 B piece c of row R stored at piece
// c ^ (2 * ((R >> 2) & 1)). A fragment is 16 consecutive rows starting at ANY
// row (the tap offset r*W + s is arbitrary); with this XOR every 16-lane
// group of a ds_read_b128 covers all 64 banks exactly once at every start
// row. (The C3_SWZ pattern of conv3x3_mfma.hip is conflict-free only at even
// start rows.)
//
// MFMA operand roles are swapped against conv3x3_mfma.hip (weights are the
// A operand, pixels the B operand), so a lane ends up with 4 consecutive
// output channels of ONE pixel per accumulator; slab row nj*16 + f holds
// output channel (f>>2)*16 + nj*4 + (f&3), which makes those 4 x 4 = 16
// consecutive channels (32 B) per lane and pixel: two 16 B stores.
#include "tfosr_common.h"
#include <cstdlib>
#include <cstring>

typedef short h_bf16x8 __attribute__((ext_vector_type(8)));
typedef float h_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int h_u32x4 __attribute__((ext_vector_type(4)));

#define H_BN 64
#define H_SLAB (9 * H_BN * 64)        // bytes: 9 taps x 64 channels x 64 B
#define H_LDS (80 * 1024)             // two workgroups per CU
#define H_MAX_ROWS ((H_LDS - H_SLAB) / 64)  // span rows that fit: 704
// byte offset inside a 512 B-aligned region
#define H_SWZ(l) ((l) ^ ((((l) >> 8) & 1) << 5))

__device__ __forceinline__ void h_stage16(const char* src,
                                          __attribute__((address_space(3))) char* dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

__device__ __forceinline__ unsigned h_pack2(float a, float b) {
  return (unsigned)__builtin_bit_cast(unsigned short, f2bf(a)) |
         ((unsigned)__builtin_bit_cast(unsigned short, f2bf(b)) << 16);
}

// WAVES waves, each 64 pixels x 64 output channels; BM = WAVES * 64.
// Requires Cin % 32 == 0 and roundup16(BM + 2*Wd + 2) <= H_MAX_ROWS.
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, WAVES / 2) void conv3x3_halo_kernel(
    const bf16_t* __restrict__ X, const bf16_t* __restrict__ W9,
    bf16_t* __restrict__ C, int Nn, int H, int Wd, int Cin, int Cout) {
  constexpr int BM = WAVES * 64;
  __shared__ __attribute__((aligned(1024))) char lds[H_LDS];
  __attribute__((address_space(3))) char* slab =
      (__attribute__((address_space(3))) char*)lds;
  __attribute__((address_space(3))) char* span = slab + H_SLAB;

  const long M = (long)Nn * H * Wd;
  const int ntn = (Cout + H_BN - 1) / H_BN;
  const int nwg = gridDim.x;
  int wgid = blockIdx.x;
  {  // consecutive tiles (shared halo rows, shared A) on one XCD
    const int q = nwg / 8, r = nwg % 8;
    const int xcd = wgid % 8, pos = wgid / 8;
    wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  const long tile_m = (long)(wgid / ntn) * BM;
  const int tile_n = (wgid % ntn) * H_BN;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fpix = lane & 15;   // fragment pixel / slab row
  const int kslot = lane >> 4;  // 16 B piece of the 64 B row

  // tap masks of this lane's four fragment pixels: bit r*3+s set when
  // (oh+r-1, ow+s-1) lies inside the pixel's own image; 0 past the end
  unsigned tapmask[4];
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const long m = tile_m + wave * 64 + mi * 16 + fpix;
    unsigned mk = 0;
    if (m < M) {
      const long rem = m % ((long)H * Wd);
      const int oh = (int)(rem / Wd), ow = (int)(rem - (long)oh * Wd);
      const unsigned rows = (oh > 0 ? 1u : 0u) | 2u | (oh < H - 1 ? 4u : 0u);
      const unsigned cols = (ow > 0 ? 1u : 0u) | 2u | (ow < Wd - 1 ? 4u : 0u);
      mk = ((rows & 1u) ? cols : 0u) | ((rows & 2u) ? cols << 3 : 0u) |
           ((rows & 4u) ? cols << 6 : 0u);
    }
    tapmask[mi] = mk;
  }

  // staging sources (per lane, chunk 0): one 1 KiB piece = 16 rows x 64 B per
  // wave-instruction, lane -> LDS byte lane*16 of the piece, which holds
  // logical piece (lane & 3) ^ swizzle of row lane >> 2
  const int nsp = (BM + 2 * Wd + 2 + 15) / 16;  // span pieces
  const int lrow = lane >> 2;
  const long first_pix = tile_m - (Wd + 1);
  const long Cinb = (long)Cin * 2;

  auto stage = [&](int cin0) {
    const long cb = (long)cin0 * 2;
    for (int p = wave; p < 36; p += WAVES) {  // slab: tap p>>2, rows (p&3)*16..
      const int l = (p & 3) * 1024 + lane * 16;
      const int col = H_SWZ(l) & 63;
      const int f = lrow;  // slab row (p&3)*16 + f <-> channel, see header
      int co = tile_n + (f >> 2) * 16 + (p & 3) * 4 + (f & 3);
      co = co < Cout ? co : Cout - 1;
      const char* src = (const char*)W9 + ((long)co * 9 + (p >> 2)) * Cinb +
                        cb + col;
      h_stage16(src, slab + p * 1024 + lane * 16);
    }
    for (int p = wave; p < nsp; p += WAVES) {
      const int l = p * 1024 + lane * 16;
      const int col = H_SWZ(l) & 63;
      long pix = first_pix + p * 16 + lrow;
      pix = pix < 0 ? 0 : (pix < M ? pix : M - 1);
      h_stage16((const char*)X + pix * Cinb + cb + col,
                span + p * 1024 + lane * 16);
    }
  };

  h_f32x4 acc[4][4];
  #pragma unroll
  for (int i = 0; i < 4; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // The swizzle looks at bit 2 of the row only, so fragments 16 rows apart
  // share one swizzled lane offset: + nj (or mi) * 1024 B is an immediate.
  const int boff = H_SWZ(fpix * 64 + kslot * 16);
  const int arow0 = wave * 64 + fpix;

  for (int cin0 = 0; cin0 < Cin; cin0 += 32) {
    stage(cin0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // r stays a real loop: unrolled, the 36 swizzled span addresses of all
    // nine taps are hoisted out of the chunk loop and spill at 128 VGPRs
    #pragma unroll 1
    for (int r = 0; r < 3; ++r) {
      #pragma unroll
      for (int s = 0; s < 3; ++s) {
        const int tap = r * 3 + s;
        const int toff = r * Wd + s;
        h_bf16x8 bfrag[4], afrag[4];
        #pragma unroll
        for (int nj = 0; nj < 4; ++nj)
          bfrag[nj] = *(__attribute__((address_space(3))) h_bf16x8*)(
              slab + tap * (H_BN * 64) + nj * 1024 + boff);
        const int l = (arow0 + toff) * 64 + kslot * 16;
        const int aoff = H_SWZ(l);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          const h_bf16x8 a = *(__attribute__((address_space(3))) h_bf16x8*)(
              span + aoff + mi * 1024);
          const h_bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
          afrag[mi] = ((tapmask[mi] >> tap) & 1u) ? a : z;
        }
        __builtin_amdgcn_s_setprio(1);
        #pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          #pragma unroll
          for (int nj = 0; nj < 4; ++nj)
            acc[mi][nj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bfrag[nj], afrag[mi], acc[mi][nj], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    if (cin0 + 32 < Cin) {  // every wave has read this chunk before the next
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }

  // lane: pixel fpix of each mi; channels tile_n + kslot*16 + nj*4 + r
  const int n0 = tile_n + kslot * 16;
  const bool vec = (Cout % 8) == 0;
  #pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const long m = tile_m + wave * 64 + mi * 16 + fpix;
    if (m >= M) continue;
    bf16_t* dst = C + m * Cout + n0;
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int nb = n0 + h * 8;
      if (vec && nb + 7 < Cout) {
        h_u32x4 v;
        v[0] = h_pack2(acc[mi][2 * h][0], acc[mi][2 * h][1]);
        v[1] = h_pack2(acc[mi][2 * h][2], acc[mi][2 * h][3]);
        v[2] = h_pack2(acc[mi][2 * h + 1][0], acc[mi][2 * h + 1][1]);
        v[3] = h_pack2(acc[mi][2 * h + 1][2], acc[mi][2 * h + 1][3]);
        *(h_u32x4*)(dst + h * 8) = v;
      } else {
        #pragma unroll
        for (int e = 0; e < 8; ++e)
          if (nb + e < Cout)
            dst[h * 8 + e] = f2bf(acc[mi][2 * h + (e >> 2)][e & 3]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host: eligibility, routing, launch
// ---------------------------------------------------------------------------

// `auto` routes a launch to the halo kernel only for a shape class that
// tools/conv_bench.py --halo measured ahead of the im2col kernel by more than
// both sides' spreads (docs/performance.md, "Halo-staged 3x3 stride-1
// kernel"). min_m is the smallest M at which the class was measured ahead; it
// also keeps the small launches of the test suites on the im2col kernel.
struct HaloClass { int Cin, Cout, W; long min_m; };
static const HaloClass kHaloAuto[] = {
    {64, 64, 56, 64L * 56 * 56},
    {128, 128, 28, 32L * 28 * 28},
    {256, 256, 14, 1024L * 14 * 14},
    {512, 512, 7, 1024L * 7 * 7},
};

// Tile height: 512 pixels where the span fits (W <= 95) and the launch still
// has a workgroup for every CU, else 256 (measured: 512 ahead from 276
// workgroups up, 256 ahead at 49 and 98). forced (256 or 512, from
// TFOS_CONV3X3_HALO_BM under TFOS_CONV3X3_TILE=halo) replaces that rule
// where its span fits. 0: the row is too wide for LDS.
static int halo_bm(long M, int W, int Cout, int forced) {
  auto fits = [&](int bm) { return (bm + 2 * W + 2 + 15) / 16 * 16 <= H_MAX_ROWS; };
  if (forced && fits(forced)) return forced;
  if (fits(512) &&
      (M + 511) / 512 * ((Cout + H_BN - 1) / H_BN) >= TFOSR_CU)
    return 512;
  if (fits(256)) return 256;
  return 0;
}

extern "C" {

// mode of TFOS_CONV3X3_TILE: 0 auto, 1 im2col, 2 halo, -1 invalid
int tfosr_conv3x3_tile_mode() {
  const char* e = getenv("TFOS_CONV3X3_TILE");
  if (!e || !*e || !strcmp(e, "auto")) return 0;
  if (!strcmp(e, "im2col")) return 1;
  if (!strcmp(e, "halo")) return 2;
  return -1;
}

// Plan of one conv_mfma launch under the current environment. eligible_launch
// is the caller's verdict on everything but the shape (3x3, stride 1, padding
// 1, no dilation of either kind, bf16 non-accumulating output of the natural
// size). Returns 1 for the halo kernel, 0 for the im2col kernel, -1 for an
// invalid TFOS_CONV3X3_TILE, -2 for a TFOS_CONV3X3_HALO_BM other than 256 or
// 512 under TFOS_CONV3X3_TILE=halo (the only mode that reads it). out: BM,
// BN, tiles, grid, largest eligible W.
int tfosr_conv3x3_halo_plan(int eligible_launch, int N, int H, int W, int Cin,
                            int Cout, int* out_bm, int* out_bn,
                            long* out_tiles, long* out_grid, int* out_max_w) {
  const int mode = tfosr_conv3x3_tile_mode();
  *out_bm = *out_bn = *out_max_w = 0;
  *out_tiles = *out_grid = 0;
  int forced = 0;
  if (mode == 2) {
    const char* e = getenv("TFOS_CONV3X3_HALO_BM");
    if (e && *e) {
      forced = !strcmp(e, "256") ? 256 : !strcmp(e, "512") ? 512 : -1;
      if (forced < 0) return -2;
    }
  }
  *out_max_w = (H_MAX_ROWS - 256 - 2) / 2;
  const long M = (long)N * H * W;
  const int bm = halo_bm(M, W, Cout, forced);
  bool halo = mode != 1 && eligible_launch && bm > 0 && Cin % 32 == 0 &&
              Cin >= 32 && Cout >= 1 && M > 0;
  if (halo && mode == 0) {
    halo = false;
    for (const HaloClass& c : kHaloAuto)
      if (c.Cin == Cin && c.Cout == Cout && c.W == W && M >= c.min_m)
        halo = true;
  }
  if (halo) {
    *out_bm = bm;
    *out_bn = H_BN;
    *out_tiles = (M + bm - 1) / bm * ((Cout + H_BN - 1) / H_BN);
    *out_grid = *out_tiles;  // one workgroup per tile
  } else {  // launch_conv's tiles (conv3x3_mfma.hip)
    *out_bm = 256;
    *out_bn = Cout >= 192 ? 256 : 128;
    *out_tiles = (M + 255) / 256 * ((Cout + *out_bn - 1) / *out_bn);
    *out_grid = *out_tiles;
  }
  return mode < 0 ? -1 : (halo ? 1 : 0);
}

// The caller has a plan that returned 1 with this bm.
void tfosr_conv3x3_halo(const void* X, const void* W9, void* Y, int bm, int N,
                        int H, int W, int Cin, int Cout, hipStream_t s) {
  const long M = (long)N * H * W;
  const long grid = (M + bm - 1) / bm * ((Cout + H_BN - 1) / H_BN);
  if (bm == 512)
    hipLaunchKernelGGL((conv3x3_halo_kernel<8>), dim3((unsigned)grid),
                       dim3(512), 0, s, (const bf16_t*)X, (const bf16_t*)W9,
                       (bf16_t*)Y, N, H, W, Cin, Cout);
  else
    hipLaunchKernelGGL((conv3x3_halo_kernel<4>), dim3((unsigned)grid),
                       dim3(256), 0, s, (const bf16_t*)X, (const bf16_t*)W9,
                       (bf16_t*)Y, N, H, W, Cin, Cout);
}

}  // extern "C"
