// The FP8 token format of a stored library (mgsv_amd/library.py, csrc/fp8.hip), in integer arithmetic on the bit patterns: one int8
// power-of-two exponent per row of D bf16 values and one OCP e4m3fn byte per value.  Plain C++ (no float operation, no intrinsic
// beyond a count of leading zeros), so that the same functions compile for the device and for a host program that checks them
// against another implementation of the contract over every bf16 pattern.
#pragma once

#include <stdint.h>

#ifndef MADE_FP8_FN
#ifdef __HIPCC__
#define MADE_FP8_FN __host__ __device__ __forceinline__
#else
#define MADE_FP8_FN static inline
#endif
#endif

MADE_FP8_FN int fp8_top_bit(uint32_t x) { return 31 - __builtin_clz(x); }      // floor(log2 x), x > 0

// The row's exponent from the bits of amax = max |x| (a bf16 pattern with the sign cleared): the smallest e with amax * 2^-e <= 448,
// clamped to [-120, 120]; 0 for a row of zeros.  amax = m * 2^ex with m in [0.5, 1): e = ex - 9 if m <= 0.875, else ex - 8.  A normal
// bf16 is (128 + M) / 256 * 2^(E - 126), so m <= 0.875 is M <= 96; a subnormal amax is below 2^-126 and always clamps.
MADE_FP8_FN int fp8_row_exponent(uint32_t amax_bits) {
    if (amax_bits == 0u) return 0;
    const int E = (int)(amax_bits >> 7), M = (int)(amax_bits & 0x7Fu);
    if (E == 0) return -120;
    const int e = E - 126 - (M <= 96 ? 9 : 8);
    return e < -120 ? -120 : (e > 120 ? 120 : e);
}

// e4m3fn(x * 2^-e), round to nearest, ties to even, with subnormals; -0 keeps its sign.  x = sig * 2^pw exactly (sig the 8-bit
// significand); the scaled value's quantum is 2^qe with qe = max(its binade, -6) - 3, n = sig * 2^(pw - e - qe) rounded to an integer
// is 8 .. 16 for a normal result and 0 .. 8 for a subnormal one, and (qe + 10) * 8 + n - 8 is the code in both cases (n = 16 and
// n = 8 carry into the exponent field by themselves).  The contract keeps |x * 2^-e| <= 448; anything larger saturates to 448.
MADE_FP8_FN uint32_t fp8_encode(uint32_t x_bits, int e) {
    const uint32_t s = (x_bits >> 8) & 0x80u;
    const int E = (int)((x_bits >> 7) & 0xFFu), M = (int)(x_bits & 0x7Fu);
    const uint32_t sig = E ? (uint32_t)(128 | M) : (uint32_t)M;
    if (sig == 0u) return s;
    const int t = (E ? E : 1) - 134 - e;                       // x * 2^-e = sig * 2^t
    const int k = fp8_top_bit(sig) + t;                        // its binade
    if (k > 8) return s | 0x7Eu;
    const int qe = (k < -6 ? -6 : k) - 3;
    int sh = qe - t;                                           // n = sig / 2^sh
    uint32_t n;
    if (sh <= 0) {
        n = sig << -sh;                                        // exact (n <= 15: k <= 8 bounds it)
    } else {
        if (sh > 10) sh = 10;                                  // sig < 2^8: everything from 2^10 on rounds to 0
        n = (sig + (1u << (sh - 1)) - 1u + ((sig >> sh) & 1u)) >> sh;
    }
    const uint32_t code = (uint32_t)((qe + 10) * 8) + n - 8u;
    return s | (code > 0x7Eu ? 0x7Eu : code);
}

// bf16(q) * 2^e as a bf16 pattern: exact (3 significand bits into 7; a result below 2^-126 is a bf16 subnormal with bits to spare).
// The e4m3fn NaN codes give a NaN and a value past the bf16 range an infinity; neither arises from fp8_encode's output.
MADE_FP8_FN uint32_t fp8_decode(uint32_t q, int e) {
    const uint32_t s = (q & 0x80u) << 8;
    const int E = (int)((q >> 3) & 0xFu);
    uint32_t M = q & 7u;
    if ((q & 0x7Fu) == 0x7Fu) return s | 0x7FC0u;
    int u;                                                     // value = (8 + M) / 8 * 2^u
    if (E == 0) {
        if (M == 0u) return s;
        const int p = fp8_top_bit(M);                          // M * 2^-9 = (M / 2^p) * 2^(p - 9)
        M = (M << (3 - p)) & 7u;
        u = p - 9;
    } else {
        u = E - 7;
    }
    const int b = u + e + 127;                                 // the biased bf16 exponent
    if (b >= 255) return s | 0x7F80u;
    if (b >= 1) return s | ((uint32_t)b << 7) | (M << 4);
    if (b < -3) return s;                                      // (an exponent below -120, which no row has)
    return s | ((8u + M) << (b + 3));                          // subnormal: (8 + M) * 2^(u + e - 3) in units of 2^-133; b >= -2 for e >= -120
}

// Four payload bytes (byte i of w = element i) -> two dwords of two bf16 patterns each.  A byte with a non-zero exponent field is a
// normal number whose bf16 pattern is its 7 low bits shifted into place plus (120 + e) in the exponent field -- for all four at once,
// no carry can cross (the sum stays below 2^15 for e <= 112).  A dword that holds a zero, a subnormal or a NaN code, or an exponent
// out of that range, takes fp8_decode element by element; a dword of zeros (padded rows) is its sign bits.
MADE_FP8_FN void fp8_decode4(uint32_t w, int e, uint32_t* lo, uint32_t* hi) {
    const uint32_t mag = w & 0x7F7F7F7Fu;
    const uint32_t sl = ((w & 0x80u) << 8) | ((w & 0x8000u) << 16), sh = ((w >> 8) & 0x8000u) | (w & 0x80000000u);
    if (mag == 0u) { *lo = sl; *hi = sh; return; }
    const uint32_t ex = mag & 0x78787878u, nn = mag ^ 0x7F7F7F7Fu;
    const uint32_t special = (((ex - 0x01010101u) & ~ex) | ((nn - 0x01010101u) & ~nn)) & 0x80808080u;      // some byte of ex or nn is zero
    if (special != 0u || (uint32_t)(e + 120) > 232u) {
        *lo = fp8_decode(w & 0xFFu, e) | (fp8_decode((w >> 8) & 0xFFu, e) << 16);
        *hi = fp8_decode((w >> 16) & 0xFFu, e) | (fp8_decode(w >> 24, e) << 16);
        return;
    }
    const uint32_t bias = (uint32_t)(120 + e) << 7, bias2 = bias | (bias << 16);
    *lo = sl | ((((mag & 0x7Fu) << 4) | ((mag & 0x7F00u) << 12)) + bias2);
    *hi = sh | ((((mag >> 12) & 0x7F0u) | ((mag >> 4) & 0x7F00000u)) + bias2);
}
