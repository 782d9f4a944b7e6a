// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's constants and
// round function) and the map from one of its words to an Exp(1) variate -- the per-request noise of the seeded sampler
// (mh_sample_top_p_k_seeded, mh_sample_noise_seeded; loss_optim.hip).  Plain C++: a round is two 32 x 32 -> 64 multiplies
// (__umulhi + a 32-bit multiply each) and four XORs; nothing here reads or writes memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace philox {

constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;  // the two round multipliers
constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;  // the key schedule (Weyl increments: golden ratio, sqrt(3) - 1)

struct U4 {
  uint32_t x, y, z, w;
};

// counter c, key (k0, k1) -> four words; round r runs on key + r * (W0, W1)
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += W0;
    k1 += W1;
  }
  return c;
}

// The variate of (request seed, event index ctr, token position pos, rank lane): word 0 of
// Philox4x32-10(counter = (ctr, pos, lane, 0), key = (seed low, seed high)), its top 23 bits n taken as the odd multiple
// u = (2 n + 1) 2^-24 of 2^-24 -- 24 significant bits, exact in fp32, in [2^-24, 1 - 2^-24], never 0 and never 1 -- and
// q = -log(u) with the accurate logf: q in [5.96e-8, 16.64], never 0, infinite or NaN.  *bits receives the word.
__device__ __forceinline__ float exp1_variate(uint64_t seed, int32_t ctr, int pos, int lane, uint32_t* bits) {
  const U4 r = philox4x32_10(U4{(uint32_t)ctr, (uint32_t)pos, (uint32_t)lane, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
  *bits = r.x;
  const uint32_t n = r.x >> 9;
  const float u = (float)(2u * n + 1u) * 0x1p-24f;
  return -logf(u);
}

}  // namespace philox
