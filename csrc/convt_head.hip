// Transposed-conv head for few classes on gfx950: ConvTranspose2d with kernel
// 4, stride 2, padding 1 (OH = 2H, OW = 2W), Cin % 8 == 0 in [8, 256], Cout
// in [1, 8], on channels_last bf16 activations. Forward, backward-data and
// weight + bias gradient.
//
// The layer is memory-bound (2 GFLOP against ~48 MB per direction at the
// U-Net's b64), and its GEMM has a tiny class axis: every kernel here runs
// v_mfma_f32_16x16x32_bf16 over the *tap* axis instead. With
// n = co * 16 + ky * 4 + kx the module's fp32 weight [Cin, Cout, 4, 4] is
// already the row-major GEMM operand W[ci][n], 16 * Cout wide, so one N tile
// is one class and nothing is packed on the host: the kernels read the
// parameter directly (scalar 4 B loads: it may be a view into a flat DDP
// bucket) and round it to bf16, nearest even, while staging it into LDS in
// MFMA fragment order (one ds_read_b128 per fragment, no bank conflicts).
//
//   geometry  oy = 2 iy - 1 + ky: an even output row takes ky in {1, 3}, an
//             odd one ky in {0, 2}; columns likewise; 2 x 2 live taps per
//             output pixel, fewer at the border.
//
//   fwd       input-centric GEMM + col2im in LDS. A workgroup (4 waves) owns
//             CT_FT x CT_FT (14 x 14) input pixels plus a one-pixel halo: 16
//             tile rows of 16 pixels, one M tile each, four per wave. The x
//             fragments (pixel = lane & 15, 8 channels at (lane >> 4) * 8 of
//             the K step: one 16 B load) are loaded once per tile and stay in
//             registers; channels past Cin and pixels outside the image are
//             masked to zero, never read; tile rows outside the image skip
//             their loads and MFMAs. Per class: P[pix][tap] = X . W_co goes
//             to LDS in fp32 (pixel stride 20 floats: the four lane groups
//             land on four bank quarters), then each of the 28 x 28 output
//             pixels adds its four P entries and the fp32 bias, rounds once
//             to bf16 and lands in an LDS output tile [28][28 * Cout]. After
//             the last class the tile's rows are stored: every output row is
//             one contiguous run of 28 * Cout bf16 that is only 2 B aligned
//             (Cout = 3, odd W), so the run is cut on the 16 B grid of the
//             address itself: whole chunks go as 16 B stores, the ragged
//             ends as 2 B stores.
//   dgrad     a workgroup owns 8 rows x 16 input pixels and stages the 18 x
//             34 x Cout dy patch tile in LDS (16 B loads on the address grid,
//             2 B at the ends, zero outside the image). M = 16 pixels of a
//             row, K = 16 * Cout padded to 32 (k = co * 16 + tap, built from
//             LDS), N = Cin in tiles of 16. Each wave owns two rows; per N
//             tile the fp32 fragment is rounded to bf16, turned in a
//             wave-private LDS block and written as 16 B vectors.
//   wrw       dw[ci][n] = sum_pix x[pix][ci] * patch[pix][n], K = pixels, in
//             two deterministic stages. A workgroup walks its slab of the
//             flat (n, iy, ix) list 32 pixels at a time: x goes to LDS as
//             row-major [32 m][16 c] blocks with 16 B loads and comes back
//             through ds_read_b64_tr_b16 as the k-major A fragment (lane
//             semantics as measured for conv_wrw2.hip); the patch fragment
//             is gathered once per block into LDS in fragment order. Wave w
//             owns channel blocks w, w + 4, ...; the threads that gather the
//             centre taps {5, 6, 9, 10} (which tile the output exactly once)
//             also add up dy for the bias gradient. Every block writes an
//             fp32 [Cin][16 Cout] + [Cout] partial; the finalize adds the
//             partials in index order. No atomics, same bits every run.
//
// Weights that do not fit the LDS budget (CT_W_PERSIST KB of fragments:
// Cin > 96 with Cout = 8, say) are restaged per class (fwd) or per N tile
// (dgrad) instead of once per workgroup.
//
// Every global access is predicated on its own bounds; grids are capped at
// TFOSR_MAX_GRID (wrw: CT_WRW_MAX_BLOCKS) with a stride loop for the rest.
#include "tfosr_common.h"

typedef unsigned int u32;
typedef short ct_s16x4 __attribute__((ext_vector_type(4)));
typedef short ct_bf16x8 __attribute__((ext_vector_type(8)));
typedef float ct_f32x4 __attribute__((ext_vector_type(4)));

#define CT_AS3 __attribute__((address_space(3)))

#define CT_BLOCK 256
#define CT_FT 14              // fwd: interior input pixels per tile side
#define CT_FH 16              //      with the halo: one M tile per tile row
#define CT_FO (2 * CT_FT)     //      output pixels per tile side
#define CT_PSTRIDE 20         //      floats per pixel of P (16 taps + pad)
#define CT_DH 8               // dgrad: input rows per tile (two per wave)
#define CT_DW 16              //        input pixels per tile row
#define CT_DYH (2 * CT_DH + 2)   //     dy tile rows
#define CT_DYW (2 * CT_DW + 2)   //     dy tile columns
#define CT_W_PERSIST 24       // KB of weight fragments kept for a block's life
#define CT_WRW_KSTEP 32       // wrw: pixels per K step
#define CT_WRW_MIN_PIX 512    //      pixels per slab before splitting
#define CT_WRW_MAX_BLOCKS 512
#define CT_FIN_OUT 32         // finalize: outputs per block ...
#define CT_FIN_LANES 8        // ... and partial slices per output
#define CT_MAX_CIN 256
#define CT_MAX_COUT 8

__device__ __forceinline__ short ct_bits(float v) {
  union { bf16_t b; short s; } u;
  u.b = f2bf(v);
  return u.s;
}

__device__ __forceinline__ float ct_val(short s) {
  union { bf16_t b; short s; } u;
  u.s = s;
  return bf2f(u.b);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// Fragments of W[ci][co * 16 + tap] for class `co` into slot `slot` of wl:
// wl[(slot * KS + ks) * 512 + lane * 8 + e] = bf16(w[ci][co][tap]) with
// ci = ks * 32 + (lane >> 4) * 8 + e, tap = lane & 15; zero past Cin.
template <int KS>
__device__ __forceinline__ void ct_fwd_stage_w(const float* __restrict__ w,
                                               short* wl, int slot, int co,
                                               int Cin, int Cout) {
  for (int q = threadIdx.x; q < KS * 512; q += CT_BLOCK) {
    const int e = q & 7, lane = (q >> 3) & 63, ks = q >> 9;
    const int ci = ks * 32 + (lane >> 4) * 8 + e;
    float v = 0.f;
    if (ci < Cin) v = w[((size_t)ci * Cout + co) * 16 + (lane & 15)];
    wl[(slot * KS + ks) * 512 + lane * 8 + e] = ct_bits(v);
  }
}

template <int KS>
__global__ __launch_bounds__(CT_BLOCK) void convt_head_fwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ bias, bf16_t* __restrict__ y, int N, int Cin,
    int Cout, int H, int W) {
  constexpr bool PERSIST_ANY = KS <= CT_W_PERSIST;  // at Cout = 1
  constexpr int WSLOTS = PERSIST_ANY ? CT_W_PERSIST / KS : 1;
  __shared__ __attribute__((aligned(16))) short wl[WSLOTS * KS * 512];
  __shared__ float P[CT_FH * CT_FH * CT_PSTRIDE];
  __shared__ __attribute__((aligned(16))) short ot[CT_FO * CT_FO * CT_MAX_COUT];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int OH = 2 * H, OW = 2 * W;
  const int TY = (H + CT_FT - 1) / CT_FT, TX = (W + CT_FT - 1) / CT_FT;
  const u32 tiles = (u32)N * TY * TX;
  const bool persist = Cout <= WSLOTS;
  if (persist) {
    for (int co = 0; co < Cout; ++co) ct_fwd_stage_w<KS>(w, wl, co, co, Cin, Cout);
  }
  __syncthreads();

  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int tx = (int)(tile % TX);
    u32 rest = tile / TX;
    const int ty = (int)(rest % TY);
    const int n = (int)(rest / TY);
    const int a = ty * CT_FT, b = tx * CT_FT;  // first interior pixel

    // x fragments: tile rows wave * 4 + mt, pixel column lane & 15
    ct_bf16x8 af[4][KS];
    bool rowlive[4];
    #pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int iy = a - 1 + wave * 4 + mt;
      const int ix = b - 1 + (lane & 15);
      rowlive[mt] = iy >= 0 && iy < H;  // wave-uniform
      const bool pix = rowlive[mt] && ix >= 0 && ix < W;
      const size_t base = (((size_t)n * H + (pix ? iy : 0)) * W + (pix ? ix : 0)) * Cin;
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int ci0 = ks * 32 + (lane >> 4) * 8;
        ct_bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (pix && ci0 < Cin) v = *(const ct_bf16x8*)(x + base + ci0);
        af[mt][ks] = v;
      }
    }

    for (int co = 0; co < Cout; ++co) {
      if (!persist) {
        // every wave is past the fragment reads of the previous class: the
        // barrier after its gather
        ct_fwd_stage_w<KS>(w, wl, 0, co, Cin, Cout);
        __syncthreads();
      }
      const int slot = persist ? co : 0;
      ct_f32x4 acc[4];
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const ct_bf16x8 bf =
            *(const ct_bf16x8*)(wl + (slot * KS + ks) * 512 + lane * 8);
        #pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          if (rowlive[mt])
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af[mt][ks], bf, acc[mt], 0, 0, 0);
        }
      }
      // D: pixel (lane >> 4) * 4 + r of the row, tap lane & 15
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int hy = wave * 4 + mt;
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int hx = (lane >> 4) * 4 + r;
          P[(hy * CT_FH + hx) * CT_PSTRIDE + (lane & 15)] = acc[mt][r];
        }
      }
      __syncthreads();
      // col2im: output pixel (oy, ox) of the tile adds its 2 x 2 live taps
      const float bv = bias ? bias[co] : 0.f;
      for (int q = t; q < CT_FO * CT_FO; q += CT_BLOCK) {
        const int oy = q / CT_FO, ox = q % CT_FO;
        const int ky0 = (oy & 1) ? 0 : 1, kx0 = (ox & 1) ? 0 : 1;
        float s = 0.f;
        #pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
          const int ky = ky0 + 2 * dy;
          const int hy = (oy + 1 - ky) / 2 + 1;
          #pragma unroll
          for (int dx = 0; dx < 2; ++dx) {
            const int kx = kx0 + 2 * dx;
            const int hx = (ox + 1 - kx) / 2 + 1;
            s += P[(hy * CT_FH + hx) * CT_PSTRIDE + ky * 4 + kx];
          }
        }
        ot[(oy * CT_FO + ox) * Cout + co] = ct_bits(s + bv);
      }
      __syncthreads();
    }

    // store: row oy of the tile is one run of `len` bf16 starting at element
    // g0 of y; chunk c covers elements [g0 & ~7) + 8c .. + 8 of y
    const int rows = min(CT_FO, OH - 2 * a);
    const int len = min(CT_FO, OW - 2 * b) * Cout;
    constexpr int CHUNKS = (CT_FO * CT_MAX_COUT + 7) / 8 + 1;
    short* yo = (short*)y;
    for (int q = t; q < CT_FO * CHUNKS; q += CT_BLOCK) {
      const int oy = q / CHUNKS, c = q % CHUNKS;
      if (oy >= rows) continue;
      const size_t g0 = (((size_t)n * OH + 2 * a + oy) * OW + 2 * b) * Cout;
      const size_t c0 = (g0 & ~(size_t)7) + (size_t)c * 8;
      if (c0 >= g0 + len) continue;
      const short* src = ot + oy * CT_FO * Cout;  // element g0 of the run
      if (c0 >= g0 && c0 + 8 <= g0 + len) {
        const int o = (int)(c0 - g0);
        s8v v;
        #pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[o + j];
        *(s8v*)(yo + c0) = v;
      } else {
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const size_t g = c0 + j;
          if (g >= g0 && g < g0 + len) yo[g] = src[(int)(g - g0)];
        }
      }
    }
    // the next tile's first write to ot comes after a barrier that this
    // loop's threads reach only past their stores
  }
}

// ---------------------------------------------------------------------------
// backward data
// ---------------------------------------------------------------------------

// Fragments of B[k][ci] = w[ci][k], k = co * 16 + tap, for N tile `nt` into
// slot `slot`: wl[(slot * KS + ks) * 512 + lane * 8 + e] with
// k = ks * 32 + (lane >> 4) * 8 + e, ci = nt * 16 + (lane & 15).
template <int KS>
__device__ __forceinline__ void ct_dgrad_stage_w(const float* __restrict__ w,
                                                 short* wl, int slot, int nt,
                                                 int Cin, int Cout) {
  const int NP = 16 * Cout;
  for (int q = threadIdx.x; q < KS * 512; q += CT_BLOCK) {
    const int e = q & 7, lane = (q >> 3) & 63, ks = q >> 9;
    const int k = ks * 32 + (lane >> 4) * 8 + e;
    const int ci = nt * 16 + (lane & 15);
    float v = 0.f;
    if (k < NP && ci < Cin) v = w[(size_t)ci * NP + k];
    wl[(slot * KS + ks) * 512 + lane * 8 + e] = ct_bits(v);
  }
}

template <int KS>
__global__ __launch_bounds__(CT_BLOCK) void convt_head_dgrad_kernel(
    const bf16_t* __restrict__ dy, const float* __restrict__ w,
    bf16_t* __restrict__ dx, int N, int Cin, int Cout, int H, int W) {
  constexpr int WSLOTS = CT_W_PERSIST / KS;
  __shared__ __attribute__((aligned(16))) short wl[WSLOTS * KS * 512];
  __shared__ short dt[CT_DYH * CT_DYW * CT_MAX_COUT];
  __shared__ __attribute__((aligned(16))) short ob[4][2][16 * 16];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int OH = 2 * H, OW = 2 * W;
  const int NT = (Cin + 15) / 16;
  const int TY = (H + CT_DH - 1) / CT_DH, TX = (W + CT_DW - 1) / CT_DW;
  const u32 tiles = (u32)N * TY * TX;
  const bool persist = NT <= WSLOTS;
  if (persist) {
    for (int nt = 0; nt < NT; ++nt) ct_dgrad_stage_w<KS>(w, wl, nt, nt, Cin, Cout);
  }
  const short* dyi = (const short*)dy;
  short* dxo = (short*)dx;

  for (u32 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int tx = (int)(tile % TX);
    u32 rest = tile / TX;
    const int ty = (int)(rest % TY);
    const int n = (int)(rest / TY);
    const int a = ty * CT_DH, b = tx * CT_DW;
    const int oy0 = 2 * a - 1, ox0 = 2 * b - 1;  // dy tile origin

    // the previous tile's fragment builds are behind the barriers of its
    // N-tile loop
    for (int q = t; q < CT_DYH * CT_DYW * Cout; q += CT_BLOCK) dt[q] = 0;
    __syncthreads();
    const int oxlo = max(ox0, 0), oxhi = min(ox0 + CT_DYW, OW);
    const int len = (oxhi - oxlo) * Cout;
    constexpr int CHUNKS = (CT_DYW * CT_MAX_COUT + 7) / 8 + 1;
    for (int q = t; q < CT_DYH * CHUNKS; q += CT_BLOCK) {
      const int lr = q / CHUNKS, c = q % CHUNKS;
      const int oy = oy0 + lr;
      if (oy < 0 || oy >= OH) continue;
      const size_t g0 = (((size_t)n * OH + oy) * OW + oxlo) * Cout;
      const size_t c0 = (g0 & ~(size_t)7) + (size_t)c * 8;
      if (c0 >= g0 + len) continue;
      short* dst = dt + (lr * CT_DYW + (oxlo - ox0)) * Cout;  // element g0
      if (c0 >= g0 && c0 + 8 <= g0 + len) {
        const s8v v = *(const s8v*)(dyi + c0);
        const int o = (int)(c0 - g0);
        #pragma unroll
        for (int j = 0; j < 8; ++j) dst[o + j] = v[j];
      } else {
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const size_t g = c0 + j;
          if (g >= g0 && g < g0 + len) dst[(int)(g - g0)] = dyi[g];
        }
      }
    }
    __syncthreads();

    // patch fragments: rows wave * 2 + mt, pixel lane & 15, k = co * 16 + tap
    ct_bf16x8 af[2][KS];
    #pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int hr = wave * 2 + mt, i = lane & 15;
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int co = ks * 2 + (lane >> 5);
        const int h = (lane >> 4) & 1;
        ct_bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (co < Cout) {
          #pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int ky = 2 * h + (e >> 2), kx = e & 3;
            v[e] = dt[((2 * hr + ky) * CT_DYW + 2 * i + kx) * Cout + co];
          }
        }
        af[mt][ks] = v;
      }
    }

    for (int nt = 0; nt < NT; ++nt) {
      if (!persist) {
        __syncthreads();  // fragment reads of the previous N tile
        ct_dgrad_stage_w<KS>(w, wl, 0, nt, Cin, Cout);
      }
      __syncthreads();  // wl staged; ob of the previous N tile read
      const int slot = persist ? nt : 0;
      ct_f32x4 acc[2];
      acc[0] = {0.f, 0.f, 0.f, 0.f};
      acc[1] = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const ct_bf16x8 bf =
            *(const ct_bf16x8*)(wl + (slot * KS + ks) * 512 + lane * 8);
        #pragma unroll
        for (int mt = 0; mt < 2; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[mt][ks], bf, acc[mt], 0, 0, 0);
      }
      // D: pixel (lane >> 4) * 4 + r, channel lane & 15 of the N tile
      #pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        #pragma unroll
        for (int r = 0; r < 4; ++r)
          ob[wave][mt][((lane >> 4) * 4 + r) * 16 + (lane & 15)] =
              ct_bits(acc[mt][r]);
      }
      __syncthreads();
      {
        const int mt = lane >> 5, i = (lane & 31) >> 1, half = lane & 1;
        const int iy = a + wave * 2 + mt, ix = b + i;
        const int ci = nt * 16 + half * 8;
        if (iy < H && ix < W && ci < Cin) {
          const s8v v = *(const s8v*)(&ob[wave][mt][i * 16 + half * 8]);
          *(s8v*)(dxo + (((size_t)n * H + iy) * W + ix) * Cin + ci) = v;
        }
      }
    }
    __syncthreads();  // before dt is cleared for the next tile
  }
}

// ---------------------------------------------------------------------------
// weight and bias gradient
// ---------------------------------------------------------------------------

// Stage one. Block b: pixels [b * slab, min(M, (b + 1) * slab)) of the flat
// (n, iy, ix) list. part is [gridDim.x][Cin * 16 * Cout + Cout].
template <int CO>
__global__ __launch_bounds__(CT_BLOCK) void convt_head_wrw_partial(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
    float* __restrict__ part, int Cin, int Cout, int H, int W, u32 M,
    u32 slab) {
  // x: [cb][32 m][16 c] row-major blocks; patch: [co][lane][8] fragments
  __shared__ __attribute__((aligned(16))) short xl[(CT_MAX_CIN / 16) * 512];
  __shared__ __attribute__((aligned(16))) short pl[CO * 512];
  __shared__ float dbred[CT_BLOCK];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int OH = 2 * H, OW = 2 * W;
  const int NP = 16 * Cout;
  const int CB = (Cin + 15) / 16;   // 16-channel blocks
  const int CV = Cin / 8;           // 16 B chunks per pixel
  const short* dyi = (const short*)dy;
  const u32 m0 = blockIdx.x * slab;
  const u32 m1 = (M - m0 < slab) ? M : m0 + slab;

  ct_f32x4 acc[4][CO];
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    #pragma unroll
    for (int c = 0; c < CO; ++c) acc[i][c] = {0.f, 0.f, 0.f, 0.f};
  }
  float dbacc[CO];
  #pragma unroll
  for (int c = 0; c < CO; ++c) dbacc[c] = 0.f;

  // a channel block with Cin % 16 == 8 has no upper half: keep it zero
  if (Cin & 8) {
    for (int q = t; q < 32 * 8; q += CT_BLOCK)
      xl[(CB - 1) * 512 + (q >> 3) * 16 + 8 + (q & 7)] = 0;
  }

  // this thread's patch element: tap and k index are fixed, see below
  const int ptap = (t >> 3) & 15, pky = ptap >> 2, pkx = ptap & 3;
  const bool centre = (pky == 1 || pky == 2) && (pkx == 1 || pkx == 2);

  // transpose-read address (bytes) into a [32 m][16 c] block: lane receives
  // channel lane & 15, pixels (lane >> 4) * 8 + 4 t + j; t = 1 sits +128 B
  const int lbase = (((lane >> 4) * 8 + ((lane & 15) >> 2)) * 16 + (lane & 3) * 4) * 2;

  for (u32 mk = m0; mk < m1; mk += CT_WRW_KSTEP) {
    // x: 32 pixels x CV chunks
    for (int q = t; q < CT_WRW_KSTEP * CV; q += CT_BLOCK) {
      const int p = q / CV, cv = q % CV;
      const u32 m = mk + p;
      s8v v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (m < m1) v = *(const s8v*)((const short*)x + (size_t)m * Cin + cv * 8);
      *(s8v*)(xl + (cv >> 1) * 512 + p * 16 + (cv & 1) * 8) = v;
    }
    // patch: element q = t + 256 u is (co = u >> 1, lane = (t >> 3) +
    // 32 (u & 1), e = t & 7): pixel (lane >> 4) * 8 + e, tap lane & 15
    #pragma unroll
    for (int u = 0; u < 2 * CO; ++u) {
      const int co = u >> 1;
      if (co < Cout) {
        const int fl = (t >> 3) + 32 * (u & 1);
        const u32 m = mk + (fl >> 4) * 8 + (t & 7);
        short s = 0;
        if (m < m1) {
          const int ix = (int)(m % W);
          u32 rest = m / W;
          const int iy = (int)(rest % H);
          const u32 n = rest / H;
          const int oy = 2 * iy - 1 + pky, ox = 2 * ix - 1 + pkx;
          if (oy >= 0 && oy < OH && ox >= 0 && ox < OW)
            s = dyi[(((size_t)n * OH + oy) * OW + ox) * Cout + co];
        }
        pl[co * 512 + fl * 8 + (t & 7)] = s;
        if (centre) dbacc[co] += ct_val(s);
      }
    }
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cb = wave + 4 * i;
      if (cb < CB) {
        CT_AS3 char* blk = (CT_AS3 char*)xl + cb * 1024 + lbase;
        const ct_s16x4 lo =
            __builtin_amdgcn_ds_read_tr16_b64_v4i16((CT_AS3 ct_s16x4*)blk);
        const ct_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (CT_AS3 ct_s16x4*)(blk + 128));
        ct_bf16x8 af;
        af[0] = lo[0]; af[1] = lo[1]; af[2] = lo[2]; af[3] = lo[3];
        af[4] = hi[0]; af[5] = hi[1]; af[6] = hi[2]; af[7] = hi[3];
        #pragma unroll
        for (int c = 0; c < CO; ++c) {
          if (c < Cout) {
            const ct_bf16x8 bf = *(const ct_bf16x8*)(pl + c * 512 + lane * 8);
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                af, bf, acc[i][c], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }

  // D: channel (lane >> 4) * 4 + r of the block, tap lane & 15
  float* po = part + (size_t)blockIdx.x * ((size_t)Cin * NP + Cout);
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cb = wave + 4 * i;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = cb * 16 + (lane >> 4) * 4 + r;
      if (cb < CB && ci < Cin) {
        #pragma unroll
        for (int c = 0; c < CO; ++c) {
          if (c < Cout) po[(size_t)ci * NP + c * 16 + (lane & 15)] = acc[i][c][r];
        }
      }
    }
  }
  // bias gradient: thread 0 adds the block's sums in thread order
  #pragma unroll
  for (int c = 0; c < CO; ++c) {
    if (c < Cout) {
      dbred[t] = dbacc[c];
      __syncthreads();
      if (t == 0) {
        float s = 0.f;
        for (int q = 0; q < CT_BLOCK; ++q) s += dbred[q];
        po[(size_t)Cin * NP + c] = s;
      }
      __syncthreads();
    }
  }
}

// Stage two: out[idx] = sum_b part[b][idx] over the nout = Cin * 16 * Cout +
// Cout values of a partial; the first ndw go to dw, the rest to db.
// CT_FIN_LANES threads per output each add every CT_FIN_LANES-th partial in
// index order, then the first adds the lane sums in lane order.
__global__ __launch_bounds__(CT_FIN_OUT * CT_FIN_LANES) void convt_head_wrw_finalize(
    const float* __restrict__ part, float* __restrict__ dw,
    float* __restrict__ db, u32 ndw, u32 nout, int nblk) {
  __shared__ float red[CT_FIN_LANES][CT_FIN_OUT];
  const int o = threadIdx.x % CT_FIN_OUT;
  const int r = threadIdx.x / CT_FIN_OUT;
  const u32 idx = blockIdx.x * CT_FIN_OUT + o;
  float s = 0.f;
  if (idx < nout) {
    for (int b = r; b < nblk; b += CT_FIN_LANES) s += part[(size_t)b * nout + idx];
  }
  red[r][o] = s;
  __syncthreads();
  if (r == 0 && idx < nout) {
    s = red[0][o];
    #pragma unroll
    for (int q = 1; q < CT_FIN_LANES; ++q) s += red[q][o];
    if (idx < ndw) dw[idx] = s;
    else db[idx - ndw] = s;
  }
}

extern "C" {

// The constants a caller (and the tests) size work from.
void tfosr_convt_head_info(int* block, int* max_grid, int* fwd_tile,
                           int* dgrad_tile_h, int* dgrad_tile_w,
                           int* w_persist_kb, int* wrw_kstep,
                           int* wrw_min_pix, int* wrw_max_blocks,
                           int* fin_lanes) {
  *block = CT_BLOCK;
  *max_grid = TFOSR_MAX_GRID;
  *fwd_tile = CT_FT;
  *dgrad_tile_h = CT_DH;
  *dgrad_tile_w = CT_DW;
  *w_persist_kb = CT_W_PERSIST;
  *wrw_kstep = CT_WRW_KSTEP;
  *wrw_min_pix = CT_WRW_MIN_PIX;
  *wrw_max_blocks = CT_WRW_MAX_BLOCKS;
  *fin_lanes = CT_FIN_LANES;
}

// How stage one of wrw splits M input pixels: one slab per CT_WRW_MIN_PIX
// pixels, capped at CT_WRW_MAX_BLOCKS slabs (the slab grows past the cap);
// the last slab may be ragged and every slab is non-empty. Cin and Cout do
// not change the split: a block covers all of both.
void tfosr_convt_head_wrw_plan(long M, int Cin, int Cout, int* nblk,
                               long* slab) {
  (void)Cin;
  (void)Cout;
  long want = (M + CT_WRW_MIN_PIX - 1) / CT_WRW_MIN_PIX;
  if (want > CT_WRW_MAX_BLOCKS) want = CT_WRW_MAX_BLOCKS;
  if (want < 1) want = 1;
  *slab = (M + want - 1) / want;
  *nblk = (int)((M + *slab - 1) / *slab);
}

void tfosr_convt_head_fwd(const void* x, const float* w, const float* bias,
                          void* y, int N, int Cin, int Cout, int H, int W,
                          hipStream_t s) {
  const long tiles = (long)N * ((H + CT_FT - 1) / CT_FT) * ((W + CT_FT - 1) / CT_FT);
  const int grid = tfosr_grid(tiles, 1);
  const int nks = (Cin + 31) / 32;
#define CT_FWD(KS)                                                            \
  hipLaunchKernelGGL((convt_head_fwd_kernel<KS>), dim3(grid), dim3(CT_BLOCK), \
                     0, s, (const bf16_t*)x, w, bias, (bf16_t*)y, N, Cin,     \
                     Cout, H, W)
  if (nks <= 1) CT_FWD(1);
  else if (nks == 2) CT_FWD(2);
  else if (nks == 3) CT_FWD(3);
  else if (nks == 4) CT_FWD(4);
  else CT_FWD(8);
#undef CT_FWD
}

void tfosr_convt_head_dgrad(const void* dy, const float* w, void* dx, int N,
                            int Cin, int Cout, int H, int W, hipStream_t s) {
  const long tiles = (long)N * ((H + CT_DH - 1) / CT_DH) * ((W + CT_DW - 1) / CT_DW);
  const int grid = tfosr_grid(tiles, 1);
  const int nks = (16 * Cout + 31) / 32;
#define CT_DGRAD(KS)                                                      \
  hipLaunchKernelGGL((convt_head_dgrad_kernel<KS>), dim3(grid),           \
                     dim3(CT_BLOCK), 0, s, (const bf16_t*)dy, w,          \
                     (bf16_t*)dx, N, Cin, Cout, H, W)
  if (nks == 1) CT_DGRAD(1);
  else if (nks == 2) CT_DGRAD(2);
  else if (nks == 3) CT_DGRAD(3);
  else CT_DGRAD(4);
#undef CT_DGRAD
}

// part: [nblk][Cin * 16 * Cout + Cout] fp32 workspace, nblk from
// tfosr_convt_head_wrw_plan. dw: [Cin, Cout, 4, 4], db: [Cout].
void tfosr_convt_head_wrw(const void* dy, const void* x, float* part,
                          float* dw, float* db, int N, int Cin, int Cout,
                          int H, int W, hipStream_t s) {
  const long M = (long)N * H * W;
  int nblk;
  long slab;
  tfosr_convt_head_wrw_plan(M, Cin, Cout, &nblk, &slab);
#define CT_WRW(CO)                                                           \
  hipLaunchKernelGGL((convt_head_wrw_partial<CO>), dim3(nblk),               \
                     dim3(CT_BLOCK), 0, s, (const bf16_t*)dy,                \
                     (const bf16_t*)x, part, Cin, Cout, H, W, (u32)M,        \
                     (u32)slab)
  if (Cout == 1) CT_WRW(1);
  else if (Cout == 2) CT_WRW(2);
  else if (Cout == 3) CT_WRW(3);
  else if (Cout == 4) CT_WRW(4);
  else CT_WRW(8);
#undef CT_WRW
  const u32 ndw = (u32)Cin * 16 * Cout, nout = ndw + Cout;
  hipLaunchKernelGGL(convt_head_wrw_finalize,
                     dim3((nout + CT_FIN_OUT - 1) / CT_FIN_OUT),
                     dim3(CT_FIN_OUT * CT_FIN_LANES), 0, s, part, dw, db, ndw,
                     nout, nblk);
}

}  // extern "C"
