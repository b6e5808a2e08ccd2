// Onsets: where a track's notes begin, from the log-mel spectrogram made_audio_fbank already computes (mgsv_amd/onsets.py).
// made_onset_strength is the spectral flux of the 128 mel bins, made_onset_peaks picks its local maxima that stand out of a moving
// mean.  The reference has no counterpart: its moments are the regressed spans as they come.
#include "common.h"

namespace {

constexpr int PEAK_TILE = 1024;         // frames one pass of a workgroup decides
constexpr int PEAK_HALO = 128;          // frames staged on either side: the largest w_avg (w_max is smaller)
constexpr int PEAK_THREADS = 256;

// Sum over a group of 32 lanes (lanes 0 .. 31 and 32 .. 63 of a wave), on the DPP path: four steps inside each row of 16 lanes, then
// lane 15 of rows 0 / 2 is added into rows 1 / 3.  Lanes 31 and 63 hold their group's total, both by the same tree.  All 64 lanes
// must be active.
__device__ __forceinline__ float half_wave_sum(float v) {
    v += dpp_f32<0xB1, 0xF>(v, v);                               // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E, 0xF>(v, v);                               // quad_perm [2,3,0,1]
    v += dpp_f32<0x124, 0xF>(v, v);                              // row_ror:4
    v += dpp_f32<0x128, 0xF>(v, v);                              // row_ror:8
    v += dpp_f32<0x142, 0xA>(0.f, v);                            // row_bcast:15 -> rows 1, 3
    return v;
}

// 32 lanes per frame, 8 frames per workgroup: lane l reads bins 4 l .. 4 l + 3 of frames f and f - lag (16 bytes each).  Frames
// outside [lag, n_frames) read nothing and write 0; every lane stays to the end (the DPP steps read their neighbours).
__global__ __launch_bounds__(256) void onset_strength_kernel(const float4* logmel, int64_t F_ld, const int32_t* n_frames, int lag,
                                                             float* env, int64_t env_ld, int tiles) {
    const int64_t t = blockIdx.x / tiles;
    const int64_t f = (int64_t)(blockIdx.x % tiles) * 8 + (threadIdx.x >> 5);
    const int l = threadIdx.x & 31;
    const int64_t nf = n_frames[t];
    const bool fits = nf >= 0 && nf <= F_ld;
    float v = 0.f;
    if (fits && f >= lag && f < nf) {
        const float4* row = logmel + (t * F_ld + f) * 32;
        const float4 a = row[l], b = row[l - (int64_t)lag * 32];
        v = (fmaxf(0.f, a.x - b.x) + fmaxf(0.f, a.y - b.y)) + (fmaxf(0.f, a.z - b.z) + fmaxf(0.f, a.w - b.w));
    }
    v = half_wave_sum(v);
    if (l == 31 && f < env_ld) env[t * env_ld + f] = fits ? v * (1.f / 128.f) : __uint_as_float(0x7FC00000u);
}

// One workgroup per track.  A pass stages frames [f0 - 128, f0 + 1024 + 128) of the envelope, every thread decides frames
// f0 + 256 j + tid for j < 4, and each j is compacted in frame order: a ballot and a prefix popcount inside the wave, the waves'
// counts through LDS, a running offset across j and the passes.
__global__ __launch_bounds__(PEAK_THREADS) void onset_peaks_kernel(const float* env, int64_t env_ld, const int32_t* n_frames, int w_max,
                                                                   int w_avg, float delta, int64_t cap, float* time, int32_t* count) {
    __shared__ float sh[PEAK_TILE + 2 * PEAK_HALO];
    __shared__ int wave_count[PEAK_THREADS / 64];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nf = n_frames[t];
    if (nf < 0 || nf > env_ld) {                                 // (uniform) a track that does not fit: no list
        if (tid == 0) count[t] = -1;
        return;
    }
    const float* e = env + t * env_ld;
    float* out = time + t * cap;
    int64_t n_out = 0;                                           // (uniform)
    for (int64_t f0 = 0; f0 < nf; f0 += PEAK_TILE) {
        __syncthreads();                                         // the pass before has read sh
        for (int i = tid; i < PEAK_TILE + 2 * PEAK_HALO; i += PEAK_THREADS) {
            const int64_t g = f0 - PEAK_HALO + i;
            sh[i] = (g >= 0 && g < nf) ? e[g] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < PEAK_TILE / PEAK_THREADS; ++j) {
            const int64_t f = f0 + j * PEAK_THREADS + tid;
            bool peak = false;
            if (f < nf) {
                const int c = PEAK_HALO + j * PEAK_THREADS + tid;                    // sh[c] = e[f]
                const float x = sh[c];
                peak = x > 0.f;
                const int lo = (int)(f - w_max < 0 ? f : w_max), hi = (int)(f + w_max >= nf ? nf - 1 - f : w_max);
                for (int d = 1; d <= lo; ++d) peak = peak && x > sh[c - d];
                for (int d = 1; d <= hi; ++d) peak = peak && x >= sh[c + d];
                if (peak) {                                      // few frames get here: at most one in w_max + 1
                    const int a = (int)(f - w_avg < 0 ? f : w_avg), b = (int)(f + w_avg >= nf ? nf - 1 - f : w_avg);
                    float s = 0.f;
                    for (int d = -a; d <= b; ++d) s += sh[c + d];                    // ascending frames
                    peak = x >= s / (float)(a + b + 1) + delta;
                }
            }
            const uint64_t m = __ballot(peak);
            if (lane == 0) wave_count[wave] = __popcll(m);
            __syncthreads();
            int64_t at = n_out;
            int total = 0;
            for (int w = 0; w < PEAK_THREADS / 64; ++w) {
                at += w < wave ? wave_count[w] : 0;
                total += wave_count[w];
            }
            at += __popcll(m & ((1ull << lane) - 1ull));
            if (peak && at < cap) out[at] = (float)f * 0.01f;
            n_out += total;
            __syncthreads();                                     // wave_count is rewritten by the next j
        }
    }
    if (tid == 0) count[t] = (int32_t)(n_out < cap ? n_out : cap);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int made_onset_strength(const float* logmel, int64_t F_ld, const int32_t* n_frames, int64_t N, int32_t lag, float* env,
                                   int64_t env_ld, void* stream) {
    MADE_REQUIRE(N >= 0 && F_ld >= 0 && env_ld >= 0, "made_onset_strength: negative size");
    MADE_REQUIRE(lag >= 1 && lag <= 8, "made_onset_strength: lag must lie in [1, 8], got %d", (int)lag);
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && (env || env_ld == 0) && (logmel || F_ld == 0), "made_onset_strength: null pointer");
    MADE_REQUIRE(aligned16(logmel), "made_onset_strength: logmel must be 16-byte aligned");
    if (env_ld == 0) return MADE_OK;
    const int64_t tiles = (env_ld + 7) / 8;
    MADE_REQUIRE(F_ld < (1LL << 31) && env_ld < (1LL << 31) && N * tiles < (1LL << 31), "made_onset_strength: too many frames for one call");
    hipLaunchKernelGGL(onset_strength_kernel, dim3((unsigned)(N * tiles)), dim3(256), 0, (hipStream_t)stream, (const float4*)logmel, F_ld,
                       n_frames, (int)lag, env, env_ld, (int)tiles);
    return made_check_launch("made_onset_strength");
}

extern "C" int made_onset_peaks(const float* env, int64_t env_ld, const int32_t* n_frames, int64_t N, int32_t w_max, int32_t w_avg,
                                float delta, int64_t cap, float* time, int32_t* count, void* stream) {
    MADE_REQUIRE(N >= 0 && env_ld >= 0 && cap >= 0, "made_onset_peaks: negative size");
    MADE_REQUIRE(w_max >= 1 && w_max <= 32, "made_onset_peaks: w_max must lie in [1, 32], got %d", (int)w_max);
    MADE_REQUIRE(w_avg >= 1 && w_avg <= PEAK_HALO, "made_onset_peaks: w_avg must lie in [1, %d], got %d", PEAK_HALO, (int)w_avg);
    MADE_REQUIRE(delta >= 0.f && delta < INFINITY, "made_onset_peaks: delta must be finite and >= 0");
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && count && (env || env_ld == 0) && (time || cap == 0), "made_onset_peaks: null pointer");
    MADE_REQUIRE(cap >=(env_ld + w_max) / (w_max + 1), "made_onset_peaks: cap must be >= ceil(env_ld / (w_max + 1)) = %lld, got %lld",
                 (long long)((env_ld + w_max) / (w_max + 1)), (long long)cap);
    MADE_REQUIRE(N < (1LL << 31) && env_ld < (1LL << 31), "made_onset_peaks: too many tracks or frames for one call");
    hipLaunchKernelGGL(onset_peaks_kernel, dim3((unsigned)N), dim3(PEAK_THREADS), 0, (hipStream_t)stream, env, env_ld, n_frames, (int)w_max,
                       (int)w_avg, delta, cap, time, count);
    return made_check_launch("made_onset_peaks");
}
