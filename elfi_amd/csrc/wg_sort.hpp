// A sort by the whole workgroup: wg_sort_u64(key, P, tid, T) sorts P = 2^k (k >= 0) 64-bit keys in LDS in ascending order
// with T threads, by a bitonic network.  Every thread of the workgroup must call it with the same arguments; the keys must
// be visible (a barrier behind the last store) and are visible when it returns.
//
// Key number i lives at key[wg_sort_slot(i)], slot(i) = i + (i >> 4): one unused word after every 16, so the buffer holds
// wg_sort_words(P) = P + P / 16 words.  A lane takes 16 consecutive keys into registers (below); at a pitch of 17 words the
// 32 lanes of a half wavefront read 32 different bank pairs, at a pitch of 16 they would share two.
//
// The network's (log2 P)(log2 P + 1) / 2 compare-exchange steps -- step (k, j) pairs key i with key i + j, ascending where
// bit k of i is clear -- are grouped so that a key travels through LDS as seldom as possible:
//   * the steps j = 8, 4, 2, 1 of every k, and all steps of k <= 16, are made on 16 keys in a lane's registers;
//   * the steps j >= 16 are taken two at a time: a lane holds keys i, i + j / 2, i + j, i + 3 j / 2 and makes steps j and j / 2.
// One barrier per pass: 29 for P = 4096, where one step per pass takes 78.  P < 16 takes the plain network.
//
// Non-negative doubles, +inf included, order as their 64-bit integer images, so a column of |x| sorts as integers and the
// compare-exchange is one 64-bit comparison; a caller pads its n values to P with the image of +inf, which the network
// leaves behind them.  NaN has no place in that order: callers drop it first (as np.nanquantile does).
//
// One lane sorting one short column (lane_sort.hpp: gnk.hip, series.hip: M/G/1, daycare.hip) stays the form for columns of a few dozen
// values, many per workgroup; this one is for ONE column of thousands per workgroup (toad.hip: 4 092 displacements).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#ifndef ELFIHIP_WG_BARRIER
#define ELFIHIP_WG_BARRIER() __syncthreads()
#endif

namespace elfihip {

#define ELFIHIP_F64_INF_BITS 0x7FF0000000000000ull

typedef unsigned long long wg_key;

__host__ __device__ inline int wg_sort_padded(int n) {
  int P = 1;
  while (P < n) P <<= 1;
  return P;
}
__host__ __device__ inline int wg_sort_slot(int i) { return i + (i >> 4); }
__host__ __device__ inline int wg_sort_words(int P) { return P + (P >> 4); }

__host__ __device__ __forceinline__ void wg_cmpx(wg_key& a, wg_key& b, bool up) {
  const wg_key lo = a < b ? a : b, hi = a < b ? b : a;
  a = up ? lo : hi;
  b = up ? hi : lo;
}

// steps j = J, J / 2, .., 1 of stage k on 16 keys in registers; `up` as the caller decides per key index
template <int J, class Up>
__host__ __device__ __forceinline__ void wg_merge16(wg_key (&r)[16], Up up) {
#pragma unroll
  for (int j = J; j >= 1; j >>= 1) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      wg_cmpx(r[i], r[i + j], up(i));
    }
  }
}

__host__ __device__ __forceinline__ void wg_sort_u64(wg_key* key, int P, int tid, int T) {
  if (P < 16) {
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j >= 1; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += T) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          wg_key a = key[i], b = key[i + j];      // (slot(i) = i below 16)
          wg_cmpx(a, b, (i & k) == 0);
          key[i] = a;
          key[i + j] = b;
        }
        ELFIHIP_WG_BARRIER();
      }
    }
    return;
  }
  // stages k = 2 .. 16 inside every block of 16 keys
  for (int c = tid; c < (P >> 4); c += T) {
    wg_key* p = key + 17 * c;
    const bool up16 = ((c << 4) & 16) == 0;
    wg_key r[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) r[i] = p[i];
    wg_merge16<1>(r, [](int i) { return (i & 2) == 0; });
    wg_merge16<2>(r, [](int i) { return (i & 4) == 0; });
    wg_merge16<4>(r, [](int i) { return (i & 8) == 0; });
    wg_merge16<8>(r, [up16](int) { return up16; });
#pragma unroll
    for (int i = 0; i < 16; ++i) p[i] = r[i];
  }
  ELFIHIP_WG_BARRIER();
  for (int k = 32; k <= P; k <<= 1) {
    int j = k >> 1;
    // steps j and j / 2 together while both are at least 16
    for (; j >= 32; j >>= 2) {
      const int h = j >> 1;
      for (int q = tid; q < (P >> 2); q += T) {
        const int i0 = ((q & ~(h - 1)) << 2) | (q & (h - 1));
        const bool up = (i0 & k) == 0;
        const int s0 = wg_sort_slot(i0), s1 = wg_sort_slot(i0 + h), s2 = wg_sort_slot(i0 + j), s3 = wg_sort_slot(i0 + j + h);
        wg_key a = key[s0], b = key[s1], c = key[s2], d = key[s3];
        wg_cmpx(a, c, up);
        wg_cmpx(b, d, up);
        wg_cmpx(a, b, up);
        wg_cmpx(c, d, up);
        key[s0] = a, key[s1] = b, key[s2] = c, key[s3] = d;
      }
      ELFIHIP_WG_BARRIER();
    }
    if (j == 16) {
      for (int t = tid; t < (P >> 1); t += T) {
        const int i = ((t & ~15) << 1) | (t & 15);
        const int s0 = wg_sort_slot(i), s1 = wg_sort_slot(i + 16);
        wg_key a = key[s0], b = key[s1];
        wg_cmpx(a, b, (i & k) == 0);
        key[s0] = a, key[s1] = b;
      }
      ELFIHIP_WG_BARRIER();
    }
    // steps 8, 4, 2, 1 in registers
    for (int c = tid; c < (P >> 4); c += T) {
      wg_key* p = key + 17 * c;
      const bool up = ((c << 4) & k) == 0;
      wg_key r[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) r[i] = p[i];
      wg_merge16<8>(r, [up](int) { return up; });
#pragma unroll
      for (int i = 0; i < 16; ++i) p[i] = r[i];
    }
    ELFIHIP_WG_BARRIER();
  }
}

}  // namespace elfihip
