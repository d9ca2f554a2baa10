// Pointwise (1x1, stride 1, no bias) convolutions for the MobileNetV2 widths
// on gfx950: channels_last bf16 activations, so [M = N*H*W, C] is the storage
// itself, channel counts that are multiples of 8 in [8, 960], and the module's
// own [Cout, Cin, 1, 1] parameter (fp32 or bf16) as the weight operand.
//
// These layers are memory-bound (16 -> 96 at b1024: 940 MB against 13 GFLOP)
// and their widths are ragged (16, 24, 144, ...), so nothing here is a
// compute-tiled GEMM: the weight stays in LDS, every activation byte is
// touched once, and ragged K, Co and M are lane predicates, never copies.
//
//   gemm   out[m][n] = sum_k in[m][k] * B[n][k], one kernel for forward
//          (in = x, B[n][k] = w[n][k]) and dgrad (in = dy, B[n][k] = w[k][n]:
//          the panel is staged transposed, two strides select which).
//
//          weight   read once per block with scalar loads (the parameter may
//                   be a view into a flat DDP bucket), rounded to bf16 nearest
//                   even and written to LDS in MFMA fragment order: fragment
//                   (tile, ks) is 64 lanes x 8 bf16, one ds_read_b128 each.
//                   Output channels are grouped in 32-channel pairs of 16-row
//                   tiles; row i of tile j of a pair is channel
//                   (i >> 2) * 8 + j * 4 + (i & 3) of the pair, so that a
//                   lane's accumulators of the two tiles are 8 consecutive
//                   channels. grid.y splits the pairs into panels when weight
//                   and activation tile together pass PW_LDS_BUDGET.
//          x tile   TM pixels x all of K is one contiguous span of memory:
//                   thread t takes 16 B chunks t, t + 256, ... of the span
//                   (fully coalesced), keeps the *next* tile's chunks in
//                   registers while the MFMAs of the current one run, and
//                   writes them to LDS rows padded by 16 B (no bank conflict
//                   between the 16 pixels of a fragment read). Chunks past M
//                   are zeros, never loads. TM is 64 up to K = 384 and 32
//                   above (a 960-wide tile of 64 would leave no room for the
//                   weight); PRE is the chunks per thread of a tile.
//          MFMA     v_mfma_f32_16x16x32_bf16 with the weight fragment as A
//                   and the pixel fragment as B: D[r] of a lane is channel
//                   (lane >> 4) * 4 + r of the tile at pixel lane & 15. A
//                   wave owns 16 pixels; per pass it carries two pairs (four
//                   accumulators) through K with one pixel-fragment read per
//                   K step, and stores 16 B per pair and pixel. With TM = 32
//                   the two wave pairs take alternate passes.
//          ragged   K fragments at or past K are zero on both sides (the
//                   weight by staging, the pixels by lane predicate: the LDS
//                   row behind them is a neighbour's, possibly NaN); channels
//                   at or past Co are zero rows that are never stored; rows
//                   at or past M are zero chunks that are never stored.
//
// There is no weight-gradient kernel here: a thin-shape wrw kernel (whole dW
// in the block's accumulators, transpose reads from LDS, two deterministic
// stages) was written and measured, and was never faster than conv_wrw2 by
// more than its spread (docs/performance.md "Pointwise convolutions"), so it
// was taken out again; PointwiseConv sends wrw to conv_wrw2 or the library.
//
// Every global access is predicated on its own bounds.
#include "tfosr_common.h"

typedef unsigned int u32;
typedef float pw_f32x4 __attribute__((ext_vector_type(4)));

#define PW_BLOCK 256
#define PW_TM 64                   // pixels per M tile (K <= PW_TM_WIDE_K)
#define PW_TM_WIDE 32              // ... and above
#define PW_TM_WIDE_K 384
#define PW_MAX_C 960
#define PW_LDS_BUDGET (152 * 1024) // weight panel + x tile, under a CU's 160 KB
#define PW_ROW_PAD 8               // bf16 of padding per LDS row of the x tile

__device__ __forceinline__ short pw_bits(float v) {
  union { bf16_t b; short s; } u;
  u.b = f2bf(v);
  return u.s;
}

// ---------------------------------------------------------------------------
// forward and dgrad
// ---------------------------------------------------------------------------

// out[M][Co] = in[M][K] . B^T with B[n][k] = w[n * sn + k * sk]. Block
// (bx, by): M tiles bx, bx + gridDim.x, ...; channel pairs [by * ppp,
// min(NP, (by + 1) * ppp)). Dynamic LDS: wl[ppp * 2 * KS * 512] then
// xl[TM * (K + PW_ROW_PAD)], both bf16.
template <int TM, int PRE>
__global__ __launch_bounds__(PW_BLOCK) void pwconv_gemm_kernel(
    const short* __restrict__ in, const void* __restrict__ w, int w_bf16,
    short* __restrict__ out, u32 M, int K, int Co, int sn, int sk, int ppp) {
  extern __shared__ __attribute__((aligned(16))) short pw_lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int KS = (K + 31) / 32;
  const int NP = (Co + 31) / 32;
  const int pair0 = blockIdx.y * ppp;
  const int npair = min(ppp, NP - pair0);
  short* wl = pw_lds;
  short* xl = pw_lds + ppp * 2 * KS * 512;
  const int XS = K + PW_ROW_PAD;        // LDS row stride of the x tile
  const int CV = K / 8;                 // 16 B chunks per pixel
  const u32 tiles = (M + TM - 1) / TM;

  // weight panel, once per block
  for (int q = t; q < npair * 2 * KS * 512; q += PW_BLOCK) {
    const int e = q & 7, l = (q >> 3) & 63, rest = q >> 9;
    const int ks = rest % KS, tj = rest / KS;
    const int i = l & 15;
    const int n = (pair0 + (tj >> 1)) * 32 + (i >> 2) * 8 + (tj & 1) * 4 + (i & 3);
    const int k = ks * 32 + (l >> 4) * 8 + e;
    float v = 0.f;
    if (n < Co && k < K) {
      const size_t idx = (size_t)n * sn + (size_t)k * sk;
      v = w_bf16 ? bf2f(((const bf16_t*)w)[idx]) : ((const float*)w)[idx];
    }
    wl[q] = pw_bits(v);
  }

  // chunk c of a tile is 16 B at element m0 * K + c * 8 of `in`
  s8v pre[PRE];
  auto fetch = [&](u32 tile) {
    const u32 m0 = tile * TM;
    const u32 live = (u32)min((u32)TM, M - m0) * CV;   // chunks inside M
    const short* src = in + (size_t)m0 * K;
    #pragma unroll
    for (int i = 0; i < PRE; ++i) {
      const u32 c = t + i * PW_BLOCK;
      s8v v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (c < live) v = *(const s8v*)(src + (size_t)c * 8);
      pre[i] = v;
    }
  };

  constexpr int WPIX = TM / 16;          // waves along the pixels of a tile
  constexpr int NSPLIT = 4 / WPIX;       // waves sharing one 16-pixel block
  const int pb = wave % WPIX;
  const int g4 = lane >> 4, px = lane & 15;

  u32 tile = blockIdx.x;
  if (tile < tiles) fetch(tile);
  while (tile < tiles) {
    __syncthreads();   // the previous tile's fragment reads; first: wl staged
    #pragma unroll
    for (int i = 0; i < PRE; ++i) {
      const int c = t + i * PW_BLOCK;
      if (c < TM * CV) *(s8v*)(xl + (c / CV) * XS + (c % CV) * 8) = pre[i];
    }
    __syncthreads();
    const u32 next = tile + gridDim.x;
    if (next < tiles) fetch(next);       // in flight under the MFMAs below

    const u32 m = tile * TM + pb * 16 + px;
    const short* xrow = xl + (pb * 16 + px) * XS + g4 * 8;
    for (int p0 = (wave / WPIX) * 2; p0 < npair; p0 += 2 * NSPLIT) {
      const bool two = p0 + 1 < npair;   // wave-uniform
      pw_f32x4 acc[4];
      #pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = {0.f, 0.f, 0.f, 0.f};
      const short* wf = wl + (p0 * 2 * KS) * 512 + lane * 8;
      for (int ks = 0; ks < KS; ++ks) {
        s8v xf = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ks * 32 + g4 * 8 < K) xf = *(const s8v*)(xrow + ks * 32);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *(const s8v*)(wf + ks * 512), xf, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *(const s8v*)(wf + (KS + ks) * 512), xf, acc[1], 0, 0, 0);
        if (two) {
          acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              *(const s8v*)(wf + (2 * KS + ks) * 512), xf, acc[2], 0, 0, 0);
          acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              *(const s8v*)(wf + (3 * KS + ks) * 512), xf, acc[3], 0, 0, 0);
        }
      }
      // acc[2 u + j][r]: channel (pair0 + p0 + u) * 32 + g4 * 8 + j * 4 + r
      #pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int n = (pair0 + p0 + u) * 32 + g4 * 8;
        if (m < M && n < Co && (u == 0 || two)) {
          s8v o;
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            o[r] = pw_bits(acc[2 * u][r]);
            o[4 + r] = pw_bits(acc[2 * u + 1][r]);
          }
          *(s8v*)(out + (size_t)m * Co + n) = o;
        }
      }
    }
    tile = next;
  }
}

extern "C" {

void tfosr_pwconv_info(int* tile_m, int* max_grid, int* max_channels) {
  *tile_m = PW_TM;
  *max_grid = TFOSR_MAX_GRID;
  *max_channels = PW_MAX_C;
}

// How a product over M pixels with K input and Co output channels is
// launched: tile_m pixels per M tile, m_tiles of them, `panels` channel
// panels of `ppp` 32-channel pairs, grid x panels blocks of lds_bytes.
void tfosr_pwconv_plan(long M, int K, int Co, int* tile_m, long* m_tiles,
                       int* panels, int* ppp, int* grid, int* lds_bytes) {
  const int TM = K <= PW_TM_WIDE_K ? PW_TM : PW_TM_WIDE;
  const int KS = (K + 31) / 32, NP = (Co + 31) / 32;
  const int xbytes = TM * (K + PW_ROW_PAD) * 2;
  const int pair_bytes = 2 * KS * 1024;
  int fit = (PW_LDS_BUDGET - xbytes) / pair_bytes;   // >= 1 at K = 960
  if (fit > NP) fit = NP;
  *tile_m = TM;
  *m_tiles = (M + TM - 1) / TM;
  *ppp = fit;
  *panels = (NP + fit - 1) / fit;
  *grid = tfosr_grid(*m_tiles, 1);
  *lds_bytes = fit * pair_bytes + xbytes;
}

// fwd: in = x, K = Cin, Co = Cout, transposed = 0. dgrad: in = dy, K = Cout,
// Co = Cin, transposed = 1. w is the [Cout, Cin] parameter either way.
hipError_t tfosr_pwconv_gemm(const void* in, const void* w, int w_bf16,
                             void* out, long M, int K, int Co, int transposed,
                             hipStream_t s) {
  int tm, panels, ppp, grid, lds;
  long m_tiles;
  tfosr_pwconv_plan(M, K, Co, &tm, &m_tiles, &panels, &ppp, &grid, &lds);
  const int sn = transposed ? 1 : K, sk = transposed ? Co : 1;
  const int pre = (tm * (K / 8) + PW_BLOCK - 1) / PW_BLOCK;
  hipError_t err = hipSuccess;
#define PW_GEMM(TM, PRE)                                                      \
  do {                                                                        \
    auto kern = pwconv_gemm_kernel<TM, PRE>;                                  \
    if (lds > 64 * 1024) { /* opt-in, per device: asked for every time */     \
      err = hipFuncSetAttribute((const void*)kern,                            \
                                hipFuncAttributeMaxDynamicSharedMemorySize,   \
                                PW_LDS_BUDGET);                               \
      if (err != hipSuccess) return err;                                      \
    }                                                                         \
    hipLaunchKernelGGL(kern, dim3(grid, panels), dim3(PW_BLOCK), lds, s,      \
                       (const short*)in, w, w_bf16, (short*)out, (u32)M, K,   \
                       Co, sn, sk, ppp);                                      \
  } while (0)
  if (tm == PW_TM) {
    if (pre <= 1) PW_GEMM(PW_TM, 1);
    else if (pre <= 2) PW_GEMM(PW_TM, 2);
    else if (pre <= 3) PW_GEMM(PW_TM, 3);
    else if (pre <= 6) PW_GEMM(PW_TM, 6);
    else PW_GEMM(PW_TM, 12);
  } else {
    if (pre <= 9) PW_GEMM(PW_TM_WIDE, 9);
    else PW_GEMM(PW_TM_WIDE, 15);
  }
#undef PW_GEMM
  return hipGetLastError();
}

}  // extern "C"
