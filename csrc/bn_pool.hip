// BatchNorm + ReLU + MaxPool2d as one op, training forward and backward, for
// the ResNet stem on gfx950: bf16 channels_last, under the NHWC fast-path
// rules of bn_relu.hip (C % 8 == 0, 2048 % C == 0, fewer than 2^31 input
// elements, u32 index math, 16 B vectors, fixed per-thread channel slots).
//
// As three ops the stem moves the conv output x and three tensors of its
// size: y = relu(bn(x)) is written to be pooled, its gradient dy is written by
// the pool's backward to be read twice by the BN's. Here neither exists:
//   fwd       reads the window's taps of x, normalizes them in registers and
//             writes the pooled p and one index byte per element;
//   bwd_stats sums dgamma / dbeta over pooled windows: only the selected tap
//             of a window carries gradient, and y[sel] = p there;
//   bwd_dx    gathers, per input pixel, dp of the <= ceil(K/S)^2 windows that
//             selected it and applies the BN input gradient in the same pass.
// Index byte: ky * K + kx of the selected tap, or 0xFF where the window's
// maximum is not positive (ReLU passes no gradient), so that the backward
// needs neither y, nor a sign mask, nor p.
#include "tfosr_common.h"

typedef unsigned char u8;
typedef unsigned int u32;
typedef u32 u2v __attribute__((ext_vector_type(2)));

#define TFOSR_POOL_NO_OWNER 0xFFu

// this thread's 8 channels: vector i starts at channel (i * 8) % C, the same
// for every i of a grid-stride loop since 256 * 8 is a multiple of C
__device__ __forceinline__ u32 pool_channel_slot(u32 C) {
  return ((blockIdx.x * blockDim.x + threadIdx.x) * 8u) % C;
}

__device__ __forceinline__ void load8(const bf16_t* p, float* out) {
  s8v v = *(const s8v*)p;
  #pragma unroll
  for (int j = 0; j < 8; ++j)
    out[j] = __uint_as_float((u32)(unsigned short)v[j] << 16);
}

// bf16 round-to-nearest-even of a float that is not NaN, kept as a float
__device__ __forceinline__ float round_bf16(float f) {
  u32 u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return __uint_as_float(u & 0xFFFF0000u);
}

// 8 index bytes, channel j in byte j of the little-endian pair
__device__ __forceinline__ u32 idx_byte(u2v v, int j) {
  return ((j < 4 ? v.x : v.y) >> (8 * (j & 3))) & 0xFFu;
}

// One thread owns 8 channels of one pooled pixel. o = relu(bn(x)) is computed
// as bn_apply_fast does and rounded to bf16 BEFORE the comparison, so p and
// the selected tap are those of bn_apply_fast followed by maxpool_fwd_nhwc,
// ties (to the first tap in row-major order) included. o is never NaN:
// fmaxf(NaN, 0) is 0, as in the two-op path.
__global__ void bn_relu_pool_fwd(const bf16_t* __restrict__ x,
                                 bf16_t* __restrict__ p, u8* __restrict__ idx,
                                 const float* __restrict__ mean,
                                 const float* __restrict__ rstd,
                                 const float* __restrict__ w,
                                 const float* __restrict__ b, u32 total, u32 C,
                                 int H, int W, int OH, int OW, int K, int S,
                                 int P) {
  const u32 c0 = pool_channel_slot(C);
  const u32 Cv = C / 8;
  float sc[8], mu[8], sh[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = w[c0 + j] * rstd[c0 + j];
    mu[j] = mean[c0 + j];
    sh[j] = b[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    u32 rest = i / Cv;
    const u32 ow = rest % (u32)OW;
    rest /= (u32)OW;
    const u32 oh = rest % (u32)OH;
    const u32 n = rest / (u32)OH;
    // every o is >= 0 (or -0), so the first in-bounds tap always beats -1
    float best[8];
    u32 bidx[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -1.f; bidx[j] = 0; }
    const int ih0 = (int)oh * S - P, iw0 = (int)ow * S - P;
    for (int ky = 0; ky < K; ++ky) {
      const int ih = ih0 + ky;
      if (ih < 0 || ih >= H) continue;
      const u32 row = (n * (u32)H + (u32)ih) * (u32)W;
      for (int kx = 0; kx < K; ++kx) {
        const int iw = iw0 + kx;
        if (iw < 0 || iw >= W) continue;
        float v[8];
        load8(x + (size_t)(row + (u32)iw) * C + c0, v);
        const u32 tap = (u32)(ky * K + kx);
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float o =
              round_bf16(fmaxf((v[j] - mu[j]) * sc[j] + sh[j], 0.f));
          if (o > best[j]) { best[j] = o; bidx[j] = tap; }
        }
      }
    }
    s8v pv;
    u2v iv = {0u, 0u};
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      pv[j] = (short)(__float_as_uint(best[j]) >> 16);
      const u32 byte = best[j] > 0.f ? bidx[j] : TFOSR_POOL_NO_OWNER;
      if (j < 4) iv.x |= byte << (8 * j);
      else iv.y |= byte << (8 * (j - 4));
    }
    *(s8v*)(p + (size_t)i * 8) = pv;
    *(u2v*)(idx + (size_t)i * 8) = iv;
  }
}

// dgamma / dbeta summed over pooled windows: a window with an owner adds dp
// to dbeta and dp * xhat(x[owner]) to dgamma. A tap of x is loaded only where
// one of the thread's 8 channels selected it. partials[block][2C]: dgamma then
// dbeta, merged by bwd_stats_merge of bn_relu.hip.
__global__ void bn_relu_pool_bwd_stats(const bf16_t* __restrict__ x,
                                       const bf16_t* __restrict__ dp,
                                       const u8* __restrict__ idx,
                                       const float* __restrict__ mean,
                                       const float* __restrict__ rstd,
                                       float* __restrict__ partials, u32 total,
                                       u32 C, int H, int W, int OH, int OW,
                                       int K, int S, int P) {
  extern __shared__ float lds[];  // [2C]
  const u32 c0 = pool_channel_slot(C);
  const u32 Cv = C / 8;
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) lds[i] = 0.f;
  __syncthreads();
  float sg[8], sb[8], mu[8], rs[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    sg[j] = 0.f; sb[j] = 0.f;
    mu[j] = mean[c0 + j]; rs[j] = rstd[c0 + j];
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    u32 rest = i / Cv;
    const u32 ow = rest % (u32)OW;
    rest /= (u32)OW;
    const u32 oh = rest % (u32)OH;
    const u32 n = rest / (u32)OH;
    float dv[8];
    load8(dp + (size_t)i * 8, dv);
    const u2v iv = *(const u2v*)(idx + (size_t)i * 8);
    u32 sel[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      sel[j] = idx_byte(iv, j);
      if (sel[j] != TFOSR_POOL_NO_OWNER) sb[j] += dv[j];
    }
    const int ih0 = (int)oh * S - P, iw0 = (int)ow * S - P;
    for (int ky = 0; ky < K; ++ky) {
      const int ih = ih0 + ky;
      if (ih < 0 || ih >= H) continue;
      const u32 row = (n * (u32)H + (u32)ih) * (u32)W;
      for (int kx = 0; kx < K; ++kx) {
        const int iw = iw0 + kx;
        if (iw < 0 || iw >= W) continue;
        const u32 tap = (u32)(ky * K + kx);
        bool any = false;
        #pragma unroll
        for (int j = 0; j < 8; ++j) any |= sel[j] == tap;
        if (!any) continue;
        float xv[8];
        load8(x + (size_t)(row + (u32)iw) * C + c0, xv);
        #pragma unroll
        for (int j = 0; j < 8; ++j)
          if (sel[j] == tap) sg[j] += dv[j] * ((xv[j] - mu[j]) * rs[j]);
      }
    }
  }
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    atomicAdd(&lds[c0 + j], sg[j]);
    atomicAdd(&lds[C + c0 + j], sb[j]);
  }
  __syncthreads();
  float* out = partials + (size_t)blockIdx.x * 2 * C;
  for (u32 i = threadIdx.x; i < 2 * C; i += blockDim.x) out[i] = lds[i];
}

// Gather, as maxpool_bwd_nhwc: per input pixel, g = sum of dp over the windows
// that selected it (fp32, not rounded to bf16 on the way), then
// dx = w * rstd * (g - dbeta / M - xhat * dgamma / M).
__global__ void bn_relu_pool_bwd_dx(const bf16_t* __restrict__ x,
                                    const bf16_t* __restrict__ dp,
                                    const u8* __restrict__ idx,
                                    bf16_t* __restrict__ dx,
                                    const float* __restrict__ mean,
                                    const float* __restrict__ rstd,
                                    const float* __restrict__ w,
                                    const float* __restrict__ dg,
                                    const float* __restrict__ db, u32 total,
                                    u32 C, int H, int W, int OH, int OW, int K,
                                    int S, int P, float invM) {
  const u32 c0 = pool_channel_slot(C);
  const u32 Cv = C / 8;
  float sc[8], mu[8], rs[8], dgm[8], dbm[8];
  #pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = mean[c0 + j]; rs[j] = rstd[c0 + j];
    sc[j] = w[c0 + j] * rs[j];
    dgm[j] = dg[c0 + j] * invM;
    dbm[j] = db[c0 + j] * invM;
  }
  const u32 stride = gridDim.x * blockDim.x;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    u32 rest = i / Cv;
    const u32 iw = rest % (u32)W;
    rest /= (u32)W;
    const u32 ih = rest % (u32)H;
    const u32 n = rest / (u32)H;
    float g[8], xv[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    load8(x + (size_t)i * 8, xv);
    // windows (oh, ow) with oh*S - P <= ih < oh*S - P + K
    int oh_lo = ((int)ih + P - K + S) / S;  // ceil((ih+P-K+1)/S)
    if (oh_lo < 0) oh_lo = 0;
    int oh_hi = ((int)ih + P) / S;
    if (oh_hi >= OH) oh_hi = OH - 1;
    int ow_lo = ((int)iw + P - K + S) / S;
    if (ow_lo < 0) ow_lo = 0;
    int ow_hi = ((int)iw + P) / S;
    if (ow_hi >= OW) ow_hi = OW - 1;
    for (int oh = oh_lo; oh <= oh_hi; ++oh) {
      const int ky = (int)ih - (oh * S - P);
      if (ky < 0 || ky >= K) continue;
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int kx = (int)iw - (ow * S - P);
        if (kx < 0 || kx >= K) continue;
        const size_t off =
            (size_t)(((n * (u32)OH + (u32)oh) * (u32)OW + (u32)ow) * C + c0);
        const u32 want = (u32)(ky * K + kx);
        const u2v iv = *(const u2v*)(idx + off);
        float dv[8];
        load8(dp + off, dv);
        #pragma unroll
        for (int j = 0; j < 8; ++j)
          if (idx_byte(iv, j) == want) g[j] += dv[j];
      }
    }
    s8v out;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float xhat = (xv[j] - mu[j]) * rs[j];
      union { short s; bf16_t h; } u;
      u.h = (bf16_t)(sc[j] * (g[j] - dbm[j] - xhat * dgm[j]));
      out[j] = u.s;
    }
    *(s8v*)(dx + (size_t)i * 8) = out;
  }
}

extern "C" {

// Does the fused stem tail take a bf16 channels_last (N, C, H, W) tensor
// pooled with K, S, P (geometry already validated by the caller)? The tap
// index K*K - 1 must stay below the no-owner byte.
int tfosr_bn_pool_eligible(long N, long C, long H, long W, long K) {
  const long total = N * C * H * W;
  return total > 0 && total < (1L << 31) && C % 8 == 0 && 2048 % C == 0 &&
         K * K <= (long)TFOSR_POOL_NO_OWNER;
}

// blocks of the backward reduction = rows of its partials[nb][2C]: red_grid's
// policy of bn_relu.hip, >= 32 pooled vectors per thread within [64, 1024]
int tfosr_bn_pool_blocks(long pooled_total) {
  long g = pooled_total / 8 / (256 * 32);
  if (g < 64) g = 64;
  if (g > 1024) g = 1024;
  return (int)g;
}

void tfosr_bn_relu_pool_fwd(const void* x, void* p, unsigned char* idx,
                            const float* mean, const float* rstd,
                            const float* w, const float* b, int N, int C,
                            int H, int W, int OH, int OW, int K, int S, int P,
                            hipStream_t s) {
  const long total = (long)N * OH * OW * (C / 8);
  if (total == 0) return;
  hipLaunchKernelGGL(bn_relu_pool_fwd, dim3(tfosr_grid(total, 256)), dim3(256),
                     0, s, (const bf16_t*)x, (bf16_t*)p, idx, mean, rstd, w, b,
                     (u32)total, (u32)C, H, W, OH, OW, K, S, P);
}

void tfosr_bn_relu_pool_bwd_stats(const void* x, const void* dp,
                                  const unsigned char* idx, const float* mean,
                                  const float* rstd, float* partials, int nb,
                                  int N, int C, int H, int W, int OH, int OW,
                                  int K, int S, int P, hipStream_t s) {
  const long total = (long)N * OH * OW * (C / 8);
  hipLaunchKernelGGL(bn_relu_pool_bwd_stats, dim3(nb), dim3(256),
                     2 * (size_t)C * sizeof(float), s, (const bf16_t*)x,
                     (const bf16_t*)dp, idx, mean, rstd, partials, (u32)total,
                     (u32)C, H, W, OH, OW, K, S, P);
}

void tfosr_bn_relu_pool_bwd_dx(const void* x, const void* dp,
                               const unsigned char* idx, void* dx,
                               const float* mean, const float* rstd,
                               const float* w, const float* dg,
                               const float* db, int N, int C, int H, int W,
                               int OH, int OW, int K, int S, int P,
                               hipStream_t s) {
  const long total = (long)N * H * W * (C / 8);
  if (total == 0) return;
  const float invM = 1.f / (float)((long)N * H * W);
  hipLaunchKernelGGL(bn_relu_pool_bwd_dx, dim3(tfosr_grid(total, 256)),
                     dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dp, idx,
                     (bf16_t*)dx, mean, rstd, w, dg, db, (u32)total, (u32)C, H,
                     W, OH, OW, K, S, P, invM);
}

}  // extern "C"
