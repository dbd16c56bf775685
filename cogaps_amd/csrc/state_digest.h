// state_digest.h -- the data digest of a session's state-file fingerprint (cogaps_session_save_state / _load_state): one pass over the
// data of sampler A as the device holds it -- the dense model's D without its pads, or the sparse model's packed values and flag words --
// summed into one 64-bit word.  Every term is an INTEGER mix of (element index, value bits) and the sum wraps around, so the result
// depends on neither the launch geometry nor the order in which waves and workgroups finish; the arrays are the same for every input
// form of a matrix (sparse_build.h, dense_build.h), and so is the digest.
#pragma once
#include "platform.h"

#define DIGEST_BS 256
// splitmix64's finaliser over index * odd constant + value: one changed bit of either changes about half the bits of the term
CG_HD unsigned long long digest_mix(unsigned long long index, unsigned long long value)
{
    unsigned long long x = index * 0x9E3779B97F4A7C15ull + value;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// wrap-around sum of x over the wave's 64 lanes (all lanes call it): four 16-bit slices through the 32-bit wave sum -- 64 * 65535 fits --
// recombined with their weights
CG_DEVICE unsigned long long digest_wave_sum(unsigned long long x)
{
    unsigned long long s = 0;
    for (int k = 0; k < 4; ++k) s += (unsigned long long)cg_wave_sum_u32((uint32_t)(x >> (16 * k)) & 0xFFFFu) << (16 * k);
    return s;
}
// vals: `rows` vectors of N 32-bit words at a stride of `stride` words (the dense model's D: M, N, Npad; the packed values: 1, nVals,
// nVals), element e = row * N + i; flags: nFlags 64-bit words, word w counted as element rows * N + w with its own salt.  Grid-stride
// over the elements (the row and the position inside it advance by the stride's quotient and remainder: no division in the loop), a
// wave reduction, the workgroup's four wave totals through LDS, ONE atomic add per workgroup.  *out must be zero before the launch.
CG_KERNEL void CG_LAUNCH_BOUNDS(DIGEST_BS) state_digest_kernel(const uint32_t *vals, unsigned long long rows, uint32_t N, uint32_t stride,
                                                                const unsigned long long *flags, unsigned long long nFlags, unsigned long long *out)
{
    CG_SHARED unsigned long long waveTot[DIGEST_BS / 64];
    const unsigned long long nVals = rows * (unsigned long long)N;
    const unsigned long long step = (unsigned long long)cg_gdim() * DIGEST_BS, first = (unsigned long long)cg_bid() * DIGEST_BS + cg_tid();
    unsigned long long acc = 0;
    if (N) {
        const unsigned long long stepRows = step / N; const uint32_t stepEl = (uint32_t)(step % N);
        unsigned long long row = first / N; uint32_t i = (uint32_t)(first % N);
        for (unsigned long long e = first; e < nVals; e += step) {
            acc += digest_mix(e, vals[row * stride + i]);
            row += stepRows; i += stepEl;
            if (i >= N) { i -= N; ++row; }
        }
    }
    for (unsigned long long w = first; w < nFlags; w += step) acc += digest_mix(nVals + w, flags[w] ^ 0xF1A65F1A65F1A65Full);
    acc = digest_wave_sum(acc);
    if ((cg_tid() & 63u) == 0u) waveTot[cg_tid() >> 6] = acc;
    cg_sync();
    if (cg_tid() == 0u) {
        unsigned long long tot = 0;
        for (int w = 0; w < DIGEST_BS / 64; ++w) tot += waveTot[w];
        cg_atomic_add_u64(out, tot);
    }
}
