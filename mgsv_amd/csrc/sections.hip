// Section boundaries: where the timbre of a track changes, from its beat-synchronous spectra (mgsv_amd/sections.py).
// made_section_novelty is Foote's checkerboard novelty in its rank-one form -- the squared distance between the weighted mean of the
// L normalised beats after a beat and the L before it, no n x n matrix; made_section_pick keeps the local maxima that stand out of
// the track's mean.  Every step of the pick is one rounded f32 operation (ops.section_pick_host restates it in numpy f32 bit for
// bit: this file is built with -ffp-contract=off); include/made_hip.h states both rules and the summation orders.  The reference has
// no counterpart.
#include "common.h"

namespace {

constexpr int BINS = 128;
constexpr int SN_THREADS = 1024;        // sixteen waves: a wave takes rows of step 1, beats of step 2 (the tile is a latency chain: more waves shorten it)
constexpr int SN_WAVES = SN_THREADS / 64;
constexpr int SN_TILE = 64;             // beats of one track a workgroup decides at a time
constexpr int SN_MAX_L = 64;            // the halo: L rows before the tile and L - 1 after it (2 L rows are staged)
constexpr int SN_MAX_Y = 1024;          // blocks along a track's tiles (a block strides over the rest)

constexpr int SP_THREADS = 256;
constexpr int SP_TILE = 1024;           // beats staged per pass
constexpr int SP_HALO = 256;            // the largest w

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// one row of step 1 in a wave: lane l holds the bins l and l + 64 (v0, v1) and gets its two entries of u
__device__ __forceinline__ void unit_row(float v0, float v1, float& u0, float& u1) {
    const float m = wave_sum(v0 + v1) * (1.0f / 128.0f);
    const float x0 = v0 - m, x1 = v1 - m;
    const float q = wave_sum(x0 * x0 + x1 * x1);
    u0 = u1 = 0.f;
    if (q > 0.f && q < INFINITY) {
        const float s = sqrtf(q);
        u0 = x0 / s;
        u1 = x1 / s;
    }
}

// grid (N, y).  Block y of track blockIdx.x takes the tiles y, y + gridDim.y, ... of 64 beats.  Step 1: the rows g0 - L .. g0 + 63 + L
// of the track that exist are normalised into LDS, a wave taking two rows at a time (both loads in flight before either is reduced),
// lane l holding the bins l and l + 64: the 128 terms of the mean and of q meet as t[l] + t[l + 64] in the lane and then in
// wave_sum's tree (depth 6).  Step 2: a wave per beat of the tile, lane l the bins l and l + 64 of a and b, each one chain over i
// ascending from +0; the 128 squares of a - b meet as in step 1.  Nothing depends on the tile a beat falls in or on the track's place
// in the batch: a row's u is a function of the row alone.
__global__ __launch_bounds__(SN_THREADS) void section_novelty_kernel(const float* B, const int64_t* beat_start, int64_t total, const float* weights, int L,
                                                                     float* novelty) {
    extern __shared__ __attribute__((aligned(16))) float u_sh[];    // [SN_TILE + 2 L][128]
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = beat_start[t], r1 = beat_start[t + 1];
    const int64_t n = r1 - r0;
    if (r0 < 0 || n < 0 || r1 > total) return;                       // (uniform) a list outside B: nothing of it is read or written
    const int rows = SN_TILE + 2 * L;
    for (int64_t g0 = (int64_t)blockIdx.y * SN_TILE; g0 < n; g0 += (int64_t)gridDim.y * SN_TILE) {
        __syncthreads();                                             // the tile before has read u_sh
        for (int r = wave; r < rows; r += 2 * SN_WAVES) {
            const int rb = r + SN_WAVES;                             // the wave's second row of this step
            const int64_t ga = g0 - L + r, gb = g0 - L + rb;         // (uniform in the wave)
            const bool has_a = ga >= 0 && ga < n, has_b = rb < rows && gb >= 0 && gb < n;
            const float* ra = B + (r0 + (has_a ? ga : 0)) * BINS;    // (a row that does not exist is not read: row 0 of the track stands in, n >= 1 here)
            const float* rw = B + (r0 + (has_b ? gb : 0)) * BINS;
            const float a0 = ra[lane], a1 = ra[lane + 64], b0 = rw[lane], b1 = rw[lane + 64];
            float ua0, ua1, ub0, ub1;
            unit_row(a0, a1, ua0, ua1);
            unit_row(b0, b1, ub0, ub1);
            u_sh[r * BINS + lane] = has_a ? ua0 : 0.f;
            u_sh[r * BINS + lane + 64] = has_a ? ua1 : 0.f;
            if (rb < rows) {
                u_sh[rb * BINS + lane] = has_b ? ub0 : 0.f;
                u_sh[rb * BINS + lane + 64] = has_b ? ub1 : 0.f;
            }
        }
        __syncthreads();
        for (int j = wave; j < SN_TILE; j += SN_WAVES) {
            const int64_t k = g0 + j;                                // (uniform in the wave)
            if (k >= n) break;
            float v = 0.f;
            if (k >= L && k <= n - L) {
                const float* after = u_sh + (L + j) * BINS + lane;   // row k
                const float* before = after - BINS;                  // row k - 1
                float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
                for (int i = 0; i < L; ++i) {
                    const float w = weights[i];
                    a0 += w * after[i * BINS];
                    a1 += w * after[i * BINS + 64];
                    b0 += w * before[-i * BINS];
                    b1 += w * before[-i * BINS + 64];
                }
                const float d0 = a0 - b0, d1 = a1 - b1;
                v = wave_sum(d0 * d0 + d1 * d1);
            }
            if (lane == 0) novelty[r0 + k] = v;
        }
    }
}

// One workgroup per track.  Pass 1: the novelty is staged 1024 beats at a time and thread 0 walks the one chain of the mean.  Pass 2:
// the beats [f0 - 256, f0 + 1024 + 256) are staged, every thread decides the beats f0 + 256 j + tid for j < 4, and each j is compacted
// in beat order: a ballot and a prefix popcount inside the wave, the waves' counts through LDS, a running offset across j and the passes.
__global__ __launch_bounds__(SP_THREADS) void section_pick_kernel(const float* novelty, const int64_t* beat_start, const float* time, int64_t cap,
                                                                  int64_t total, const int32_t* metre, const int32_t* phase, int L, int w,
                                                                  float thresh_factor, float floor_v, float* bound_time, int32_t* bound_beat,
                                                                  float* bound_strength, int64_t cap_s, int32_t* bound_count, float* mean) {
    __shared__ float sh[SP_TILE + 2 * SP_HALO];
    __shared__ int wave_count[SP_THREADS / 64];
    __shared__ float mean_sh;
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = beat_start[t], r1 = beat_start[t + 1];
    const int64_t n = r1 - r0;
    if (r0 < 0 || n < 0 || r1 > total || n > cap) {                  // (uniform) a list that does not fit its arrays: nothing of it is read
        if (tid == 0) {
            bound_count[t] = -1;
            mean[t] = quiet_nan();
        }
        return;
    }
    const int m = metre ? metre[t] : 0;
    const int step = m > 0 ? m : 1;                                  // the candidates are step beats apart
    int64_t first = L;                                               // the first candidate
    if (m > 0) {
        const int64_t r = (((int64_t)L - phase[t]) % m + m) % m;
        first = L + (r ? m - r : 0);
    }
    const int64_t last = n - L;                                      // candidates are first, first + step, ... <= last
    const float* nv = novelty + r0;
    // pass 1: the mean, one chain over the candidates ascending from +0
    float s = 0.f;                                                   // (thread 0's)
    for (int64_t f0 = 0; f0 <= last; f0 += SP_TILE) {
        __syncthreads();
        for (int i = tid; i < SP_TILE; i += SP_THREADS) sh[i] = f0 + i < n ? nv[f0 + i] : 0.f;
        __syncthreads();
        if (tid == 0) {
            int64_t k = first;
            if (k < f0) k += (f0 - k + step - 1) / step * step;
            const int64_t end = last < f0 + SP_TILE - 1 ? last : f0 + SP_TILE - 1;
            for (; k <= end; k += step) s += sh[k - f0];
        }
    }
    if (tid == 0) {
        const int64_t cnt = last >= first ? (last - first) / step + 1 : 0;
        const float mu = cnt > 0 ? s / (float)cnt : quiet_nan();
        mean[t] = mu;
        mean_sh = mu;
    }
    __syncthreads();
    const float mu = mean_sh;
    const float thresh = mu * thresh_factor;
    float* out_t = bound_time + t * cap_s;
    int32_t* out_b = bound_beat + t * cap_s;
    float* out_s = bound_strength + t * cap_s;
    const float* tm = time + t * cap;
    int64_t n_out = 0;                                               // (uniform)
    for (int64_t f0 = 0; f0 <= last; f0 += SP_TILE) {
        __syncthreads();                                             // the pass before has read sh
        for (int i = tid; i < SP_TILE + 2 * SP_HALO; i += SP_THREADS) {
            const int64_t g = f0 - SP_HALO + i;
            sh[i] = (g >= 0 && g < n) ? nv[g] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < SP_TILE / SP_THREADS; ++j) {
            const int64_t k = f0 + j * SP_THREADS + tid;
            bool peak = false;
            if (k >= first && k <= last && (k - first) % step == 0) {
                const int c = SP_HALO + j * SP_THREADS + tid;        // sh[c] = novelty[k]
                const float x = sh[c];
                peak = x > 0.f && x >= floor_v && x >= thresh;
                if (peak) {
                    const int64_t lo = k - first < w ? k - first : w, hi = last - k < w ? last - k : w;
                    for (int d = step; d <= lo; d += step) peak = peak && x > sh[c - d];
                    for (int d = step; d <= hi; d += step) peak = peak && x >= sh[c + d];
                }
            }
            const uint64_t msk = __ballot(peak);
            if (lane == 0) wave_count[wave] = __popcll(msk);
            __syncthreads();
            int64_t at = n_out;
            int tot = 0;
            for (int v = 0; v < SP_THREADS / 64; ++v) {
                at += v < wave ? wave_count[v] : 0;
                tot += wave_count[v];
            }
            at += __popcll(msk & ((1ull << lane) - 1ull));
            if (peak && at < cap_s) {
                out_t[at] = tm[k];
                out_b[at] = (int32_t)k;
                out_s[at] = sh[SP_HALO + j * SP_THREADS + tid] / mu;
            }
            n_out += tot;
            __syncthreads();                                         // wave_count is rewritten by the next j
        }
    }
    if (tid == 0) bound_count[t] = n_out <= cap_s ? (int32_t)n_out : -1;
}

}  // namespace

extern "C" int made_section_novelty(const float* B, const int64_t* beat_start, int64_t N, int64_t total, const float* weights, int32_t L,
                                    float* novelty, void* stream) {
    MADE_REQUIRE(N >= 0 && total >= 0, "made_section_novelty: negative size");
    MADE_REQUIRE(L >= 1 && L <= SN_MAX_L, "made_section_novelty: L must lie in [1, %d], got %d", SN_MAX_L, (int)L);
    MADE_REQUIRE(N < (1LL << 31) && total < (1LL << 31), "made_section_novelty: too many tracks or beats for one call");
    MADE_REQUIRE(total == 0 || (B && novelty && weights && beat_start), "made_section_novelty: null pointer");
    if (N == 0 || total == 0) return MADE_OK;                        // no track can hold a beat: nothing to write
    const int lds = (SN_TILE + 2 * (int)L) * BINS * (int)sizeof(float);
    static bool attr_done = false;                                   // (more than 64 KB of dynamic LDS needs the attribute)
    if (!attr_done) {
        constexpr int LDS_MAX = (SN_TILE + 2 * SN_MAX_L) * BINS * (int)sizeof(float);
        const hipError_t e = hipFuncSetAttribute((const void*)section_novelty_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        if (e != hipSuccess) {
            made_set_error("made_section_novelty: cannot reserve %d bytes of LDS: %s", LDS_MAX, hipGetErrorString(e));
            return MADE_ERR_HIP;
        }
        attr_done = true;
    }
    const int64_t y = (total + SN_TILE - 1) / SN_TILE;
    hipLaunchKernelGGL(section_novelty_kernel, dim3((unsigned)N, (unsigned)(y < SN_MAX_Y ? y : SN_MAX_Y)), dim3(SN_THREADS), lds, (hipStream_t)stream,
                       B, beat_start, total, weights, (int)L, novelty);
    return made_check_launch("made_section_novelty");
}

extern "C" int made_section_pick(const float* novelty, const int64_t* beat_start, const float* time, int64_t cap, int64_t N, int64_t total,
                                 const int32_t* metre, const int32_t* phase, int32_t L, int32_t w, float thresh_factor, float floor,
                                 float* bound_time, int32_t* bound_beat, float* bound_strength, int64_t cap_s, int32_t* bound_count, float* mean,
                                 void* stream) {
    MADE_REQUIRE(N >= 0 && cap >= 0 && total >= 0 && cap_s >= 0, "made_section_pick: negative size");
    MADE_REQUIRE(L >= 1 && L <= SN_MAX_L, "made_section_pick: L must lie in [1, %d], got %d", SN_MAX_L, (int)L);
    MADE_REQUIRE(w >= 1 && w <= SP_HALO, "made_section_pick: w must lie in [1, %d], got %d", SP_HALO, (int)w);
    MADE_REQUIRE(thresh_factor > -INFINITY && thresh_factor < INFINITY, "made_section_pick: thresh_factor must be finite");
    MADE_REQUIRE(floor > -INFINITY && floor < INFINITY, "made_section_pick: floor must be finite");
    MADE_REQUIRE(!metre || phase, "made_section_pick: metre given without phase");
    MADE_REQUIRE(N < (1LL << 31) && total < (1LL << 31), "made_section_pick: too many tracks or beats for one call");
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(beat_start && bound_count && mean && (novelty || total == 0) && (time || cap == 0) &&
                     ((bound_time && bound_beat && bound_strength) || cap_s == 0),
                 "made_section_pick: null pointer");
    hipLaunchKernelGGL(section_pick_kernel, dim3((unsigned)N), dim3(SP_THREADS), 0, (hipStream_t)stream, novelty, beat_start, time, cap, total, metre,
                       phase, (int)L, (int)w, thresh_factor, floor, bound_time, bound_beat, bound_strength, cap_s, bound_count, mean);
    return made_check_launch("made_section_pick");
}
