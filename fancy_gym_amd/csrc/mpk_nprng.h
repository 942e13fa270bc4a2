// numpy's default generator on the device, bit for bit: np.random.default_rng(seed) is SeedSequence(seed) (pool size 4) ->
// generate_state(4, uint64) -> PCG64 (the 128-bit LCG with XSL-RR output, stepped before output; not PCG64DXSM), and the draws the
// reacher resets use (numpy/random/bit_generator.pyx, numpy/random/src/pcg64/pcg64.h, numpy/random/src/distributions/
// distributions.c: next_double, random_uniform; random_bounded_uint64_fill -> buffered_bounded_lemire_uint32 behind choice).
// The state is exactly what rng.bit_generator.state shows: (state, inc, has_uint32, uinteger) -- the 32-bit buffer is part of it.
// Host and device code.  Compiled with -ffp-contract=off: uniform() rounds hi - lo, the product and the sum separately, as numpy
// does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mpk {

// the layout of mpk_nprng_state (include/mpk.h): 5 x uint64 per episode
struct NpRng {
    uint64_t s_hi, s_lo, inc_hi, inc_lo;
    uint32_t has_uint32, uinteger;
};

// PCG_DEFAULT_MULTIPLIER_128
constexpr uint64_t kPcgMulHi = 2549297995355413924ull, kPcgMulLo = 4865540595714422341ull;

__host__ __device__ __forceinline__ uint64_t mul64hi(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// state = state * mult + inc (mod 2^128)
__host__ __device__ __forceinline__ void pcg_step(NpRng& r) {
    const uint64_t lo = r.s_lo * kPcgMulLo;
    uint64_t hi = mul64hi(r.s_lo, kPcgMulLo) + r.s_lo * kPcgMulHi + r.s_hi * kPcgMulLo;
    const uint64_t nlo = lo + r.inc_lo;
    hi = hi + r.inc_hi + (nlo < lo ? 1ull : 0ull);
    r.s_lo = nlo;
    r.s_hi = hi;
}

// pcg_setseq_128_xsl_rr_64_random_r: step, then rotr64(hi ^ lo, state >> 122)
__host__ __device__ __forceinline__ uint64_t np_next_uint64(NpRng& r) {
    pcg_step(r);
    const uint64_t x = r.s_hi ^ r.s_lo;
    const unsigned rot = (unsigned)(r.s_hi >> 58);
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// pcg64_next32: the low half of a 64-bit draw now, the high half at the next 32-bit draw
__host__ __device__ __forceinline__ uint32_t np_next_uint32(NpRng& r) {
    if (r.has_uint32) {
        r.has_uint32 = 0;
        return r.uinteger;
    }
    const uint64_t v = np_next_uint64(r);
    r.has_uint32 = 1;
    r.uinteger = (uint32_t)(v >> 32);
    return (uint32_t)v;
}

__host__ __device__ __forceinline__ double np_next_double(NpRng& r) {
    return (double)(np_next_uint64(r) >> 11) * (1.0 / 9007199254740992.0);
}

// Generator.uniform(lo, hi): lo + (hi - lo) * next_double, each operation rounded
__host__ __device__ __forceinline__ double np_uniform(NpRng& r, double lo, double hi) {
    const double range = hi - lo;
    return lo + range * np_next_double(r);
}

// Generator.choice([-1, 1]): integers(0, 2) -> Lemire's bounded draw on next_uint32 with rng = 1.  Its rejection threshold
// (UINT32_MAX - 1) % 2 is 0, so the first draw is always taken: index = (u32 * 2) >> 32.
__host__ __device__ __forceinline__ double np_choice_pm1(NpRng& r) {
    const uint64_t m = (uint64_t)np_next_uint32(r) * 2ull;
    return (m >> 32) ? 1.0 : -1.0;
}

// SeedSequence(seed).generate_state(4, uint64) (bit_generator.pyx: _coerce_to_uint32_array, mix_entropy, hashmix, mix), then
// PCG64's seeding: initstate = s0:s1, initseq = s2:s3; state = 0; inc = initseq << 1 | 1; step; state += initstate; step
__host__ __device__ __forceinline__ NpRng np_seed(uint64_t seed) {
    constexpr uint32_t kInitA = 0x43b0d7e5u, kMultA = 0x931e8875u, kInitB = 0x8b51f9ddu, kMultB = 0x58f38dedu;
    constexpr uint32_t kMixL = 0xca01f9ddu, kMixR = 0x4973f715u;
    // entropy: one 32-bit word for seeds < 2^32 (0 is one zero word), two otherwise; the pool of 4 runs the hash on zeros
    const uint32_t e0 = (uint32_t)seed, e1 = (uint32_t)(seed >> 32);
    const int n_ent = (seed >> 32) ? 2 : 1;
    uint32_t hc = kInitA;
    auto hashmix = [&](uint32_t v) {
        v ^= hc;
        hc *= kMultA;
        v *= hc;
        return v ^ (v >> 16);
    };
    auto mix = [](uint32_t x, uint32_t y) {
        uint32_t res = kMixL * x - kMixR * y;
        return res ^ (res >> 16);
    };
    uint32_t pool[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pool[i] = hashmix(i == 0 ? e0 : (i == 1 && n_ent == 2 ? e1 : 0u));
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = mix(pool[d], hashmix(pool[s]));
    uint32_t hb = kInitB, w[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3] ^ hb;
        hb *= kMultB;
        v *= hb;
        w[i] = v ^ (v >> 16);
    }
    // little-endian pairs: uint64 k = w[2k] | w[2k+1] << 32
    const uint64_t s0 = w[0] | (uint64_t)w[1] << 32, s1 = w[2] | (uint64_t)w[3] << 32;
    const uint64_t s2 = w[4] | (uint64_t)w[5] << 32, s3 = w[6] | (uint64_t)w[7] << 32;
    NpRng r;
    r.inc_hi = (s2 << 1) | (s3 >> 63);
    r.inc_lo = (s3 << 1) | 1ull;
    r.s_hi = 0; r.s_lo = 0;
    pcg_step(r);
    const uint64_t lo = r.s_lo + s1;
    r.s_hi = r.s_hi + s0 + (lo < s1 ? 1ull : 0ull);
    r.s_lo = lo;
    pcg_step(r);
    r.has_uint32 = 0; r.uinteger = 0;
    return r;
}

}  // namespace mpk
