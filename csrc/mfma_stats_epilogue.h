// BatchNorm batch statistics taken in the epilogue of the MFMA GEMM / conv
// kernels, from the accumulator tile a block is about to store (or has just
// stored), instead of by a separate pass that reads the tensor back.
//
// A block's tile is BM = WSTACK * MI * 16 rows by BN columns; a wave owns
// MI * 16 rows by 64 columns as MI x 4 fragments in the MFMA C layout: lane l
// holds column (l & 15) of each of its four 16-column groups and the rows
// mi * 16 + (l >> 4) * 4 + r, r = 0..3. Per column the block produces
//
//     part[tile_row][0][n] = mean of the tile's valid rows
//     part[tile_row][1][n] = M2, their sum of squared deviations from it
//
// over the values as rounded to bf16 (what the BN apply pass will read), with
// rows m >= M left out: the kernels clamp or redirect those source rows, so
// their accumulators hold duplicates, not zeros. Columns n >= N are not
// written. bn_relu.hip's tile merge combines the tiles with the parallel-
// variance formula.
//
// Order of the reduction, fixed so that the result is reproducible:
//   1. a lane sums d = v - k and d * d over its MI * 4 rows, four rows at a
//      time, around the shift k = its wave's first row of that column (fetched
//      from the lane that holds it): |mean| may be many sigma, so raw sums of
//      v and v * v would cancel;
//   2. two xor-shuffles add the four (l >> 4) row groups;
//   3. lanes 0..15 of each wave put (k, sum d, sum d * d) into LDS (the
//      staging ring is dead after the K loop), one barrier, and thread c of
//      the block turns the WSTACK waves of column c into (n, mean, M2) each
//      and chains them with the parallel-variance update;
//   4. that thread stores the two floats. No atomics anywhere.
#pragma once
#include "tfosr_common.h"

typedef float msf32x4 __attribute__((ext_vector_type(4)));

// LDS floats the epilogue needs: [WSTACK][3][BN]
#define TFOSR_TILE_STATS_LDS_FLOATS(WSTACK, BN) ((WSTACK) * 3 * (BN))

template <int MI, int WSTACK, int BN>
__device__ __forceinline__ void mfma_tile_stats(
    const msf32x4 (&acc)[MI][4], float* lf, int wr, int wc, int lane, int t,
    long tile_m, long tile_n, long M, int N, float* __restrict__ part_row) {
  constexpr int WM = MI * 16;
  const int ccol = lane & 15;
  const long lrow0 = tile_m + (long)wr * WM + (lane >> 4) * 4;
  float k[4], s[4], q[4];
  #pragma unroll
  for (int nj = 0; nj < 4; ++nj) {
    // a wave's first row may itself be past M: still a finite value of the
    // column, which is all a shift has to be
    k[nj] = __shfl((float)(bf16_t)acc[0][nj][0], ccol, 64);
    s[nj] = 0.f;
    q[nj] = 0.f;
  }
  #pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = lrow0 + mi * 16 + r < M;
      #pragma unroll
      for (int nj = 0; nj < 4; ++nj) {
        float d = (float)(bf16_t)acc[mi][nj][r] - k[nj];
        d = ok ? d : 0.f;
        s4[nj] += d;
        q4[nj] += d * d;
      }
    }
    #pragma unroll
    for (int nj = 0; nj < 4; ++nj) { s[nj] += s4[nj]; q[nj] += q4[nj]; }
  }
  #pragma unroll
  for (int nj = 0; nj < 4; ++nj) {
    s[nj] += __shfl_xor(s[nj], 16, 64);
    q[nj] += __shfl_xor(q[nj], 16, 64);
    s[nj] += __shfl_xor(s[nj], 32, 64);
    q[nj] += __shfl_xor(q[nj], 32, 64);
  }
  if (lane < 16) {
    #pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int col = wc * 64 + nj * 16 + ccol;
      lf[(wr * 3 + 0) * BN + col] = k[nj];
      lf[(wr * 3 + 1) * BN + col] = s[nj];
      lf[(wr * 3 + 2) * BN + col] = q[nj];
    }
  }
  __syncthreads();
  if (t < BN && tile_n + t < N) {
    float n = 0.f, mean = 0.f, m2 = 0.f;
    #pragma unroll
    for (int w = 0; w < WSTACK; ++w) {
      const long rem = M - (tile_m + (long)w * WM);
      if (rem <= 0) break;
      const float nw = (float)(rem < WM ? rem : WM);
      const float kw = lf[(w * 3 + 0) * BN + t];
      const float sw = lf[(w * 3 + 1) * BN + t];
      const float qw = lf[(w * 3 + 2) * BN + t];
      const float dm = sw / nw;
      const float mean_w = kw + dm;
      const float m2_w = fmaxf(qw - sw * dm, 0.f);
      if (w == 0) {
        n = nw; mean = mean_w; m2 = m2_w;
      } else {
        const float delta = mean_w - mean;
        const float nn = n + nw;
        mean += delta * (nw / nn);
        m2 += m2_w + delta * delta * (n * nw / nn);
        n = nn;
      }
    }
    part_row[tile_n + t] = mean;
    part_row[(long)N + tile_n + t] = m2;
  }
}
