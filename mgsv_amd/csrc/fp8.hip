// FP8 token storage of a music library (mgsv_amd/library.py dtype "fp8"): the [N, S, D] bf16 tower outputs kept as one OCP e4m3fn
// byte per value and one int8 power-of-two exponent per row of D values, and widened back to bf16 on the device in front of the
// kernels that read them.  The scale is a power of two, so the widening is exact: an FP8 library IS the bf16 library of its
// dequantised tokens.  Both kernels stream: no LDS, no atomics, no workspace; the format's arithmetic is csrc/fp8_format.h
// (integers on the bit patterns -- gfx950's conversions are OCP too, but the same functions also compile for the host, where
// tests/test_fp8_library_cpu.py holds them to torch's own e4m3fn conversion).  The reference stores f32 features only.
#include "common.h"
#include "fp8_format.h"

namespace {

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}

// max over the 16 lanes of a DPP row; every lane of the row ends with it (the first four steps of common.h wave_max)
__device__ __forceinline__ uint32_t row16_max(uint32_t v) {
    v = max(v, dpp_u32<0xB1>(v));                               // quad_perm [1,0,3,2]
    v = max(v, dpp_u32<0x4E>(v));                               // quad_perm [2,3,0,1]
    v = max(v, dpp_u32<0x124>(v));                              // row_ror:4
    v = max(v, dpp_u32<0x128>(v));                              // row_ror:8
    return v;
}

// A 16-lane group per row, NV = D / 128 16-byte loads per lane: fragment j of lane l holds elements (16 j + l) * 8 .. + 7.
// amax is the largest pattern with the sign cleared (bf16 patterns of finite values order as integers).
template <int NV>
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const uint4* __restrict__ src, int64_t R, u32x2* __restrict__ q,
                                                           int8_t* __restrict__ exp_out) {
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= R) return;                                          // (a row's 16 lanes leave together: whole DPP rows stay active)
    const int l = threadIdx.x & 15;
    const uint4* s = src + r * (NV * 16);
    uint4 x[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) x[j] = s[j * 16 + l];
    uint32_t amax = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const uint32_t w[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
#pragma unroll
        for (int i = 0; i < 4; ++i) amax = max(amax, max(w[i] & 0x7FFFu, (w[i] >> 16) & 0x7FFFu));
    }
    amax = row16_max(amax);
    const int e = fp8_row_exponent(amax);
    if (l == 0) exp_out[r] = (int8_t)e;
    u32x2* d = q + r * (NV * 16);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const uint32_t w[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
        uint32_t o[2];
#pragma unroll
        for (int h = 0; h < 2; ++h)
            o[h] = fp8_encode(w[2 * h] & 0xFFFFu, e) | (fp8_encode(w[2 * h] >> 16, e) << 8) | (fp8_encode(w[2 * h + 1] & 0xFFFFu, e) << 16) |
                   (fp8_encode(w[2 * h + 1] >> 16, e) << 24);
        u32x2 v;
        v.x = o[0]; v.y = o[1];
        d[j * 16 + l] = v;
    }
}

__device__ __forceinline__ uint4 fp8_decode8(uint32_t a, uint32_t b, int e) {
    uint4 o;
    fp8_decode4(a, e, &o.x, &o.y);
    fp8_decode4(b, e, &o.z, &o.w);
    return o;
}

// One lane per 16 values: 16 payload bytes in, two 16-byte stores out; a destination row takes D / 16 consecutive lanes.  Output row
// t is source row index[t / rpi] * rpi + t % rpi (t itself without an index); an index outside [0, U) writes zeros and reads nothing.
__global__ __launch_bounds__(256) void fp8_dequantize_kernel(const uint4* __restrict__ q, const int8_t* __restrict__ exp_in,
                                                             const int32_t* __restrict__ index, int64_t U, int64_t rows, int rpi, int f16,
                                                             uint4* __restrict__ dst) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t t = g / f16;
    if (t >= rows) return;
    const int f = (int)(g - t * f16);
    int64_t sr = t;
    if (index) {
        const int64_t c = t / rpi;
        const int64_t u = index[c];
        sr = (u >= 0 && u < U) ? u * rpi + (t - c * rpi) : -1;
    }
    uint4 lo = make_uint4(0u, 0u, 0u, 0u), hi = lo;
    if (sr >= 0) {
        const uint4 p = q[sr * f16 + f];
        const int e = exp_in[sr];
        lo = fp8_decode8(p.x, p.y, e);
        hi = fp8_decode8(p.z, p.w, e);
    }
    uint4* d = dst + (t * f16 + f) * 2;
    d[0] = lo;
    d[1] = hi;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
bool supported_width(int64_t D) { return D == 128 || D == 256 || D == 512; }
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na > 0 && nb > 0 && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace

extern "C" int made_fp8_quantize_rows(const void* src, int64_t R, int64_t D, uint8_t* q, int8_t* exp, void* stream) {
    MADE_REQUIRE(R >= 0 && R < (1LL << 31) * 16, "made_fp8_quantize_rows: bad row count");
    MADE_UNSUPPORTED(supported_width(D), "made_fp8_quantize_rows: D must be 128, 256 or 512 (got %lld)", (long long)D);
    if (R == 0) return MADE_OK;
    MADE_REQUIRE(src && q && exp, "made_fp8_quantize_rows: null pointer");
    MADE_REQUIRE(aligned16(src) && aligned16(q), "made_fp8_quantize_rows: src and q must be 16-byte aligned");
    MADE_REQUIRE(!overlap(src, R * D * 2, q, R * D) && !overlap(src, R * D * 2, exp, R) && !overlap(q, R * D, exp, R),
                 "made_fp8_quantize_rows: the outputs must not alias the input or each other");
    const dim3 grid((unsigned)((R + 15) / 16)), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (D == 128) hipLaunchKernelGGL(fp8_quantize_kernel<1>, grid, block, 0, st, (const uint4*)src, R, (u32x2*)q, exp);
    else if (D == 256) hipLaunchKernelGGL(fp8_quantize_kernel<2>, grid, block, 0, st, (const uint4*)src, R, (u32x2*)q, exp);
    else hipLaunchKernelGGL(fp8_quantize_kernel<4>, grid, block, 0, st, (const uint4*)src, R, (u32x2*)q, exp);
    return made_check_launch("made_fp8_quantize_rows");
}

extern "C" int made_fp8_dequantize_rows(const uint8_t* q, const int8_t* exp, int64_t U, const int32_t* index, int64_t R,
                                        int64_t rows_per_index, int64_t D, void* dst, void* stream) {
    MADE_REQUIRE(U >= 0 && R >= 0 && rows_per_index >= 1 && rows_per_index < (1LL << 31), "made_fp8_dequantize_rows: bad dims");
    MADE_UNSUPPORTED(supported_width(D), "made_fp8_dequantize_rows: D must be 128, 256 or 512 (got %lld)", (long long)D);
    MADE_REQUIRE(index || R <= U, "made_fp8_dequantize_rows: without an index R must be <= U");
    const int64_t rows = R * rows_per_index, f16 = D / 16;
    MADE_REQUIRE(rows < (1LL << 31) * 256 / f16, "made_fp8_dequantize_rows: too many rows for one launch");
    if (rows == 0) return MADE_OK;
    MADE_REQUIRE(dst && ((q && exp) || U == 0), "made_fp8_dequantize_rows: null pointer");
    MADE_REQUIRE(aligned16(q) && aligned16(dst), "made_fp8_dequantize_rows: q and dst must be 16-byte aligned");
    const int64_t src_rows = index ? U * rows_per_index : rows;
    MADE_REQUIRE(!overlap(dst, rows * D * 2, q, src_rows * D) && !overlap(dst, rows * D * 2, exp, src_rows) &&
                     !(index && overlap(dst, rows * D * 2, index, R * 4)),
                 "made_fp8_dequantize_rows: dst must not alias q, exp or index");
    const int64_t lanes = rows * f16;
    hipLaunchKernelGGL(fp8_dequantize_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)q, exp,
                       index, U, rows, (int)rows_per_index, (int)f16, (uint4*)dst);
    return made_check_launch("made_fp8_dequantize_rows");
}
