// Near-duplicate grouping at library build: the threshold self-join of a vector table (made_cosine_join; mgsv_amd/dedup.py).  Every
// pair (i, j), i < j, of a row range and a column range of one table whose cosine reaches tau is appended to a pair list.  The
// reference has no counterpart: its library is whatever the dataset lists.
//
// A GEMM that never stores C.  One workgroup of 256 threads (4 waves, 2 x 2) per 128 x 128 tile of the (row range) x (column range)
// rectangle; a tile whose every row index is >= its every column index exits at once.  The K loop walks D in slabs of 32: the slab
// of the 128 rows and of the 128 columns (both are rows of `vec`) comes from global memory in 16-byte loads, one slab ahead in
// registers, and goes to LDS as [256][32 + 4] f32 -- the pad makes ds_read_b128 of 16 different rows at one k cover 64 distinct
// banks (36 r mod 64 = 4 (9 r mod 16), a bijection of r mod 16; MI355X_MICROARCH.md, LDS).  A wave owns 64 x 64 = 2 x 2
// accumulator tiles of v_mfma_f32_32x32x2_f32, the exact-f32 product: lane half hh reads k = 8 s + 4 hh .. + 3 of its row in one
// ds_read_b128 and element e of both operands feeds MFMA e of the step, so a dot product is ONE fmaf chain over k in the order
// 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ... whatever the tile, the ranges or the launch: its bits depend on the two rows alone.  Thread t
// sums the squares of row t of the 256 staged rows in four chains (one per component of a 16-byte fragment, fragments ascending,
// (c0 + c1) + (c2 + c3)), so a norm depends on its row alone too.  Nothing is normalised beforehand: the epilogue divides.
//
// Epilogue: a multiply-compare pre-test with a slack of 2^-20 of |tau| |a| |b| passes every pair the division could accept, the
// division decides the few that pass.  Matches are rare, so a tile normally ends at one __syncthreads_or.  Otherwise: the threads'
// counts are prefix-summed (wave scan, then the four wave totals), ONE atomicAdd per workgroup reserves the slots on the 64-bit
// counter, and every match whose slot is < capacity is stored with ordinary vector stores.  The order of the list therefore depends
// on which workgroup reserves first; the set does not.  No inline assembly.
#include "common.h"

#include <math.h>

namespace {

constexpr int CJ_T = 256;                // threads
constexpr int CJ_BM = 128;               // tile edge
constexpr int CJ_KS = 32;                // slab depth
constexpr int CJ_LD = CJ_KS + 4;         // LDS row stride (floats)

template <int D>
__global__ __launch_bounds__(CJ_T) void cosine_join_kernel(const float* __restrict__ vec, const int32_t* __restrict__ node, int64_t r0,
                                                           int64_t r1, int64_t c0, int64_t c1, int n_row_tiles, float tau,
                                                           int32_t* pair_i, int32_t* pair_j, float* pair_cos, int64_t capacity,
                                                           unsigned long long* count) {
    __shared__ __attribute__((aligned(16))) float tile[2 * CJ_BM * CJ_LD];          // rows 0 .. 127: the row tile, 128 .. 255: the column tile
    __shared__ float norm[2 * CJ_BM];
    __shared__ int wave_total[CJ_T / WAVE];
    __shared__ unsigned long long slot_base;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1, r = lane & 31, hh = lane >> 5;
    // the row tile runs fastest: the workgroups resident together share a few column blocks (and the 64 row blocks of a strip)
    const int64_t R = r0 + (int64_t)(blockIdx.x % (unsigned)n_row_tiles) * CJ_BM;
    const int64_t C = c0 + (int64_t)(blockIdx.x / (unsigned)n_row_tiles) * CJ_BM;
    const int64_t rend = R + CJ_BM < r1 ? R + CJ_BM : r1, cend = C + CJ_BM < c1 ? C + CJ_BM : c1;
    if (R >= cend - 1) return;                                   // no i < j in this tile (block-uniform, before any barrier)

    // this thread's eight 16-byte chunks of a slab: staged row q >> 3 (8 chunks per row), chunk q & 7, q = tid + 256 t
    const float* src[8];
    bool live[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int q = tid + CJ_T * t, row = q >> 3;
        const int64_t g = row < CJ_BM ? R + row : C + (row - CJ_BM);
        live[t] = row < CJ_BM ? g < rend : g < cend;
        src[t] = vec + (live[t] ? g : (row < CJ_BM ? R : C)) * D + 4 * (q & 7);      // (R and C are rows of the table)
    }
    f32x4 pre[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) pre[t] = keep_or_zero(*reinterpret_cast<const f32x4*>(src[t]), live[t]);

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;                // squared norm of staged row tid

    for (int s = 0; s < D / CJ_KS; ++s) {
        if (s) __syncthreads();                                  // the slab before has been read
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int q = tid + CJ_T * t;
            *reinterpret_cast<f32x4*>(tile + (q >> 3) * CJ_LD + 4 * (q & 7)) = pre[t];
        }
        __syncthreads();
        if (s + 1 < D / CJ_KS) {
#pragma unroll
            for (int t = 0; t < 8; ++t) pre[t] = keep_or_zero(*reinterpret_cast<const f32x4*>(src[t] + (s + 1) * CJ_KS), live[t]);
        }
#pragma unroll
        for (int f = 0; f < CJ_KS / 4; ++f) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(tile + tid * CJ_LD + 4 * f);
            n0 = fmaf(x[0], x[0], n0);
            n1 = fmaf(x[1], x[1], n1);
            n2 = fmaf(x[2], x[2], n2);
            n3 = fmaf(x[3], x[3], n3);
        }
#pragma unroll
        for (int ks = 0; ks < CJ_KS / 8; ++ks) {
            f32x4 a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *reinterpret_cast<const f32x4*>(tile + (wr * 64 + t * 32 + r) * CJ_LD + 8 * ks + 4 * hh);
                b[t] = *reinterpret_cast<const f32x4*>(tile + (CJ_BM + wc * 64 + t * 32 + r) * CJ_LD + 8 * ks + 4 * hh);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][e], b[j][e], acc[i][j], 0, 0, 0);
        }
    }

    {
        const float sq = (n0 + n1) + (n2 + n3);
        norm[tid] = (sq > 0.f && sq < INFINITY) ? sqrtf(sq) : 0.f;                    // 0: the row joins nothing
    }
    __syncthreads();

    // accumulator (i, j, e) of this lane: row R + wr 64 + i 32 + acc_row(e, hh), column C + wc 64 + j 32 + r
    auto cosine = [&](int i, int j, int e, float& c) -> bool {
        const float den = norm[wr * 64 + i * 32 + acc_row(e, hh)] * norm[CJ_BM + wc * 64 + j * 32 + r];
        c = acc[i][j][e] / den;
        return den > 0.f && den < INFINITY && c >= tau;
    };
    uint64_t match = 0;                                          // bit (i 2 + j) 16 + e
    const float nb[2] = {norm[CJ_BM + wc * 64 + r], norm[CJ_BM + wc * 64 + 32 + r]};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t gi = R + wr * 64 + i * 32 + acc_row(e, hh);
            const float na = norm[wr * 64 + i * 32 + acc_row(e, hh)];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t gj = C + wc * 64 + j * 32 + r;
                const float td = tau * (na * nb[j]);
                // every pair the division accepts passes (the slack is 8 roundings wide); a tiny product of norms is left to the division
                if (gi < gj && gi < rend && gj < cend && (acc[i][j][e] >= td - fabsf(td) * 0x1p-20f || fabsf(td) < 0x1p-100f)) {
                    float c;
                    if (cosine(i, j, e, c) && (node == nullptr || node[gi] != node[gj])) match |= 1ull << ((i * 2 + j) * 16 + e);
                }
            }
        }
    const int mine = __popcll(match);
    if (!__syncthreads_or(mine)) return;                         // the usual end of a tile

    int incl = mine;                                             // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == WAVE - 1) wave_total[w] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
#pragma unroll
    for (int x = 0; x < CJ_T / WAVE; ++x) {
        if (x < w) before += wave_total[x];
        total += wave_total[x];
    }
    if (tid == 0) slot_base = atomicAdd(count, (unsigned long long)total);
    __syncthreads();
    int64_t slot = (int64_t)slot_base + before;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (!((match >> ((i * 2 + j) * 16 + e)) & 1ull)) continue;
                if (slot >= 0 && slot < capacity) {
                    float c;
                    cosine(i, j, e, c);
                    pair_i[slot] = (int32_t)(R + wr * 64 + i * 32 + acc_row(e, hh));
                    pair_j[slot] = (int32_t)(C + wc * 64 + j * 32 + r);
                    pair_cos[slot] = c;
                }
                ++slot;
            }
}

template <int D>
int cosine_join_launch(const float* vec, const int32_t* node, int64_t r0, int64_t r1, int64_t c0, int64_t c1, float tau, int32_t* pair_i,
                       int32_t* pair_j, float* pair_cos, int64_t capacity, int64_t* count, hipStream_t stream) {
    const int64_t nr = (r1 - r0 + CJ_BM - 1) / CJ_BM, nc = (c1 - c0 + CJ_BM - 1) / CJ_BM;
    MADE_UNSUPPORTED(nr * nc < (1LL << 31), "made_cosine_join: %lld x %lld tiles in one call, split the row range", (long long)nr,
                     (long long)nc);
    hipLaunchKernelGGL(cosine_join_kernel<D>, dim3((unsigned)(nr * nc)), dim3(CJ_T), 0, stream, vec, node, r0, r1, c0, c1, (int)nr, tau,
                       pair_i, pair_j, pair_cos, capacity, reinterpret_cast<unsigned long long*>(count));
    return made_check_launch("made_cosine_join");
}

}  // namespace

extern "C" int made_cosine_join(const float* vec, int64_t N, int64_t D, const int32_t* node, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                                float tau, int32_t* pair_i, int32_t* pair_j, float* pair_cos, int64_t capacity, int64_t* count,
                                void* stream) {
    MADE_REQUIRE(N >= 0 && N < (1LL << 31), "made_cosine_join: bad dims (0 <= N < 2^31)");
    MADE_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= N && 0 <= c0 && c0 <= c1 && c1 <= N,
                 "made_cosine_join: needs 0 <= r0 <= r1 <= N and 0 <= c0 <= c1 <= N, got rows [%lld, %lld), columns [%lld, %lld), N = %lld",
                 (long long)r0, (long long)r1, (long long)c0, (long long)c1, (long long)N);
    MADE_REQUIRE(tau > -1.f && tau <= 1.f, "made_cosine_join: tau must be in (-1, 1]");
    MADE_REQUIRE(capacity >= 0 && count != nullptr && (capacity == 0 || (pair_i && pair_j && pair_cos)), "made_cosine_join: null pointer");
    MADE_REQUIRE(vec != nullptr || N == 0, "made_cosine_join: null pointer");
    MADE_UNSUPPORTED(D == 128 || D == 256 || D == 512, "made_cosine_join: D must be 128, 256 or 512, got %lld", (long long)D);
    MADE_REQUIRE(((uintptr_t)vec & 15u) == 0, "made_cosine_join: vec must be 16-byte aligned");
    if (r0 == r1 || c0 == c1 || r0 >= c1 - 1) return MADE_OK;    // empty, or wholly on or below the diagonal
    hipStream_t st = (hipStream_t)stream;
    if (D == 128) return cosine_join_launch<128>(vec, node, r0, r1, c0, c1, tau, pair_i, pair_j, pair_cos, capacity, count, st);
    if (D == 256) return cosine_join_launch<256>(vec, node, r0, r1, c0, c1, tau, pair_i, pair_j, pair_cos, capacity, count, st);
    return cosine_join_launch<512>(vec, node, r0, r1, c0, c1, tau, pair_i, pair_j, pair_cos, capacity, count, st);
}
