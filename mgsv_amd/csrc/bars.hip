// Bar grids: the metre, the phase and the downbeats of a track, from its log-mel spectrogram and its beat list (mgsv_amd/bars.py).
// made_beat_sync_mean is the mean spectrum of every beat's interval; made_bar_pick turns the energy that arrives at every beat
// into a score per (metre, phase) and picks one.  Every step of the pick is one rounded f32 operation (ops.bar_pick_host restates
// steps 2 - 6 in numpy f32 bit for bit: this file is built with -ffp-contract=off); include/made_hip.h states both rules and both
// summation orders.  The reference has no counterpart.
#include "common.h"

namespace {

constexpr int BINS = 128;
constexpr int SM_THREADS = 256;         // four waves: a wave takes a beat
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_MAX_Y = 4096;          // blocks along a track's beats (a wave strides over the rest)

constexpr int BP_THREADS = 1024;        // sixteen waves: a wave takes a beat of step 1
constexpr int BP_WAVES = BP_THREADS / 64;
constexpr int BP_LDS_BEATS = 4096;      // beats whose evidence stays in LDS (a longer track reads it back from `evidence`)
constexpr int BP_MAX_CAND = 35;         // 2 + 3 + ... + 8 (metre, phase) pairs
constexpr int BP_MIN_METRE = 2, BP_MAX_METRE = 8;

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// the frame of a beat time, kept inside [0, nf]: (int)(t * 100 + 0.5), two rounded operations; a NaN or a negative time gives 0
__device__ __forceinline__ int beat_frame(float t, int nf) {
    const float x = t * 100.0f + 0.5f;
    return x >= 0.f ? (x < (float)nf ? (int)x : nf) : 0;
}

// grid (N, y).  Wave w of block y takes the beats k = 4 y + w, + 4 gridDim.y, ... of track blockIdx.x.  Lane l owns the bins
// 4 (l & 31) .. + 3 (one 16-byte load) of the frames of parity l >> 5: a step of the walk covers 8 frames, a lane holding four
// running sums per bin (u = 0 .. 3: the frame b + 8 i + 2 u + (l >> 5)).  So a bin has 8 chains, chain c = 2 u + h adding the frames
// b + c, b + c + 8, ... ascending, and the tree ((c0 + c2) + (c4 + c6)) + ((c1 + c3) + (c5 + c7)): inside a lane first, then across
// the two halves of the wave.  A frame past the interval adds +0 (its load is redirected to the interval's last frame: nothing past
// nf is read).
__global__ __launch_bounds__(SM_THREADS) void beat_sync_mean_kernel(const float* spec, int64_t spec_ld, const int32_t* n_frames, const float* time,
                                                                    int64_t cap, const int32_t* count, const int64_t* beat_start, int64_t total_beats,
                                                                    float* B) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
    const int64_t n = count[t];
    const int64_t nf64 = n_frames[t];
    const int64_t r0 = beat_start[t], r1 = beat_start[t + 1];
    if (n <= 0 || n > cap || nf64 < 0 || nf64 > spec_ld || r0 < 0 || r1 > total_beats || r1 - r0 != n) return;      // (uniform) nothing of the track is written
    const int nf = (int)nf64;
    const float* tm = time + t * cap;
    const f32x4* sp = (const f32x4*)(spec + t * spec_ld * BINS) + (lane & 31);
    for (int64_t k = (int64_t)blockIdx.y * SM_WAVES + wave; k < n; k += (int64_t)gridDim.y * SM_WAVES) {
        const int b = beat_frame(tm[k], nf);
        int e;
        if (k + 1 < n) e = beat_frame(tm[k + 1], nf);
        else if (n >= 2) {
            const int64_t step = (int64_t)b - beat_frame(tm[k - 1], nf);
            e = (int)(b + step < nf ? (b + step > 0 ? b + step : 0) : nf);
        } else e = b + 1 < nf ? b + 1 : nf;
        const int L = e - b;                                         // (uniform in the wave)
        float a[4][4] = {};                                          // (scalars: this library keeps packed-FP32 instructions out -- see the Makefile)
        for (int f0 = b + h; f0 < e + h; f0 += 8) {                  // (uniform trip count: f0 - h runs over b, b + 8, ...)
            f32x4 x[4];
            bool keep[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = f0 + 2 * u;
                keep[u] = f < e;
                x[u] = sp[(int64_t)(keep[u] ? f : e - 1) * (BINS / 4)];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[u][j] += keep[u] ? x[u][j] : 0.f;
        }
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float mine = (a[0][j] + a[1][j]) + (a[2][j] + a[3][j]);
            const float other = __shfl_xor(mine, 32);
            s[j] = h == 0 ? mine + other : other + mine;             // (the even frames' half on the left in both halves: the same bits)
        }
        if (h == 0) {
            f32x4 out = {0.f, 0.f, 0.f, 0.f};
            if (L > 0) {
                const float len = (float)L;
#pragma unroll
                for (int j = 0; j < 4; ++j) out[j] = s[j] / len;
            }
            ((f32x4*)(B + (r0 + k) * BINS))[lane] = out;
        }
    }
}

// One workgroup per track.  Step 1: wave w takes the beats k = 1 + w, + 16, ...; lane l the bins l and l + 64; the 128 terms meet as
// t[l] + t[l + 64] in the lane and then in wave_sum's tree over the 64 lanes (depth 6), times 1 / 128.  Steps 2 - 3: thread 0 walks
// the chain of all beats, thread 1 + c the chain of candidate c, each one sequential f32 sum over e in LDS (in `evidence` for a track
// of more than BP_LDS_BEATS beats).  Step 4: thread 0 walks the candidates in (metre, phase) order with a strict >.
__global__ __launch_bounds__(BP_THREADS) void bar_pick_kernel(const float* B, const int64_t* beat_start, const float* time, int64_t cap,
                                                              int64_t total_beats, int metre_mask, int low_bins, float low_weight, int min_bars,
                                                              float min_strength, float* evidence, int32_t* metre, int32_t* phase, float* strength,
                                                              float* down_time, int64_t cap_d, int32_t* down_count) {
    __shared__ float e_sh[BP_LDS_BEATS];
    __shared__ float sums[1 + BP_MAX_CAND];
    __shared__ int pick[3];                                          // metre, phase, number of downbeats
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = beat_start[t], r1 = beat_start[t + 1];
    const int64_t n = r1 - r0;
    if (r0 < 0 || n < 0 || r1 > total_beats || n > cap) {            // (uniform) a list that does not fit its arrays: nothing of it is read
        if (tid == 0) {
            metre[t] = 0;
            phase[t] = -1;
            strength[t] = quiet_nan();
            down_count[t] = -1;
        }
        return;
    }
    const bool in_lds = n <= BP_LDS_BEATS;
    float* ev = evidence + r0;
    const float w_lo = 1.0f + low_weight;
    const float w0 = lane < low_bins ? w_lo : 1.0f, w1 = lane + 64 < low_bins ? w_lo : 1.0f;
    if (tid == 0 && n > 0) {
        ev[0] = 0.f;
        if (in_lds) e_sh[0] = 0.f;
    }
    for (int64_t k = 1 + wave; k < n; k += BP_WAVES) {
        const float* cur = B + (r0 + k) * BINS;
        const float* prev = cur - BINS;
        const float d0 = cur[lane] - prev[lane], d1 = cur[lane + 64] - prev[lane + 64];
        const float v = wave_sum(w0 * fmaxf(0.f, d0) + w1 * fmaxf(0.f, d1)) * (1.0f / 128.0f);
        if (lane == 0) {
            ev[k] = v;
            if (in_lds) e_sh[k] = v;
        }
    }
    __threadfence();                                                 // a long track reads `evidence` back: the writes of every wave must be visible
    __syncthreads();
    // the candidates in (metre, phase) order: thread 1 + c takes candidate c
    int my_m = 0, my_phi = 0;
    {
        int c = tid - 1;
        for (int m = BP_MIN_METRE; m <= BP_MAX_METRE && tid >= 1; ++m) {
            if (!((metre_mask >> m) & 1)) continue;
            if (c >= 0 && c < m) {
                my_m = m;
                my_phi = c;
            }
            c -= m;
        }
    }
    if (tid == 0 || my_m > 0) {
        const int64_t first = tid == 0 ? 1 : (my_phi == 0 ? my_m : my_phi), step = tid == 0 ? 1 : my_m;
        float s = 0.f;
        if (in_lds)
            for (int64_t k = first; k < n; k += step) s += e_sh[k];
        else
            for (int64_t k = first; k < n; k += step) s += ev[k];
        sums[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int bm = 0, bphi = -1, nd = 0;
        float st = quiet_nan();
        if (n >= 2) {
            const float mean_all = sums[0] / (float)(n - 1);
            float best = 0.f;
            int c = 1;
            for (int m = BP_MIN_METRE; m <= BP_MAX_METRE; ++m) {
                if (!((metre_mask >> m) & 1)) continue;
                for (int phi = 0; phi < m; ++phi, ++c) {
                    const int64_t cnt = phi == 0 ? (n - 1) / m : (phi <= n - 1 ? (n - 1 - phi) / m + 1 : 0);
                    if (cnt < min_bars) continue;
                    const float score = sums[c] / (float)cnt - mean_all;
                    if (score != score) continue;
                    if (bm == 0 || score > best) {                   // strict: of equal scores the smaller metre, then the smaller phase
                        best = score;
                        bm = m;
                        bphi = phi;
                    }
                }
            }
            if (bm > 0) {
                st = best / mean_all;
                if (!(mean_all > 0.f) || !(st >= min_strength)) bm = 0;
            }
        }
        if (bm == 0) {
            bphi = -1;
            st = quiet_nan();
        } else {
            const int64_t want = (n - 1 - bphi) / bm + 1;
            nd = want <= cap_d ? (int)want : -1;
        }
        metre[t] = bm;
        phase[t] = bphi;
        strength[t] = st;
        down_count[t] = nd;
        pick[0] = bm;
        pick[1] = bphi;
        pick[2] = nd;
    }
    __syncthreads();
    const int bm = pick[0], bphi = pick[1], nd = pick[2];
    const float* tm = time + t * cap;
    float* out = down_time + t * cap_d;
    for (int i = tid; i < nd; i += BP_THREADS) out[i] = tm[bphi + (int64_t)i * bm];
}

}  // namespace

extern "C" int made_beat_sync_mean(const float* spec, int64_t spec_ld, const int32_t* n_frames, const float* time, int64_t cap, const int32_t* count,
                                   const int64_t* beat_start, int64_t N, int64_t total_beats, float* B, void* stream) {
    MADE_REQUIRE(N >= 0 && spec_ld >= 0 && cap >= 0 && total_beats >= 0, "made_beat_sync_mean: negative size");
    MADE_REQUIRE(spec_ld < (1LL << 20), "made_beat_sync_mean: spec_ld must be < 2^20 frames (a beat's frame is recovered from its f32 time), got %lld",
                 (long long)spec_ld);
    MADE_REQUIRE(N < (1LL << 31) && total_beats < (1LL << 31), "made_beat_sync_mean: too many tracks or beats for one call");
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && count && beat_start && (spec || spec_ld == 0) && (time || cap == 0) && (B || total_beats == 0),
                 "made_beat_sync_mean: null pointer");
    if (cap == 0 || total_beats == 0 || spec_ld == 0) return MADE_OK;                  // no track can hold a beat: nothing to write
    const int64_t y = (cap + SM_WAVES - 1) / SM_WAVES;
    hipLaunchKernelGGL(beat_sync_mean_kernel, dim3((unsigned)N, (unsigned)(y < SM_MAX_Y ? y : SM_MAX_Y)), dim3(SM_THREADS), 0, (hipStream_t)stream,
                       spec, spec_ld, n_frames, time, cap, count, beat_start, total_beats, B);
    return made_check_launch("made_beat_sync_mean");
}

extern "C" int made_bar_pick(const float* B, const int64_t* beat_start, const float* time, int64_t cap, int64_t N, int64_t total_beats,
                             int32_t metre_mask, int32_t low_bins, float low_weight, int32_t min_bars, float min_strength, float* evidence,
                             int32_t* metre, int32_t* phase, float* strength, float* down_time, int64_t cap_d, int32_t* down_count, void* stream) {
    MADE_REQUIRE(N >= 0 && cap >= 0 && total_beats >= 0 && cap_d >= 0, "made_bar_pick: negative size");
    MADE_REQUIRE(metre_mask != 0 && (metre_mask & ~0x1FC) == 0, "made_bar_pick: metres must be a non-empty set of integers in [2, 8] (bits 2 .. 8), got mask 0x%x",
                 (unsigned)metre_mask);
    MADE_REQUIRE(low_bins >= 0 && low_bins <= BINS, "made_bar_pick: low_bins must lie in [0, 128], got %d", (int)low_bins);
    MADE_REQUIRE(low_weight >= 0.f && low_weight < INFINITY, "made_bar_pick: low_weight must be finite and >= 0");
    MADE_REQUIRE(min_bars >= 1, "made_bar_pick: min_bars must be >= 1, got %d", (int)min_bars);
    MADE_REQUIRE(min_strength >= 0.f && min_strength < INFINITY, "made_bar_pick: min_strength must be finite and >= 0");
    MADE_REQUIRE(cap_d >= (cap + 1) / 2, "made_bar_pick: cap_d must be >= ceil(cap / 2) = %lld (every second beat may be a downbeat), got %lld",
                 (long long)((cap + 1) / 2), (long long)cap_d);
    MADE_REQUIRE(N < (1LL << 31) && total_beats < (1LL << 31), "made_bar_pick: too many tracks or beats for one call");
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(beat_start && metre && phase && strength && down_count && ((B && evidence) || total_beats == 0) && (time || cap == 0) &&
                     (down_time || cap_d == 0),
                 "made_bar_pick: null pointer");
    hipLaunchKernelGGL(bar_pick_kernel, dim3((unsigned)N), dim3(BP_THREADS), 0, (hipStream_t)stream, B, beat_start, time, cap, total_beats,
                       (int)metre_mask, (int)low_bins, low_weight, (int)min_bars, min_strength, evidence, metre, phase, strength, down_time, cap_d,
                       down_count);
    return made_check_launch("made_bar_pick");
}
