// Beat grids: one tempo and the beat times of a track, from made_onset_strength's 10 ms envelope (mgsv_amd/beats.py).
// made_tempo_autocorr is the mean-removed autocorrelation of the envelope over a band of lags and the pick of the period under a
// tempo prior; made_beat_track is Ellis's dynamic programme over the envelope with that period, every step one rounded f32
// operation (tests/beats_ref.py restates it in numpy f32 bit for bit: this file is built with -ffp-contract=off).  The reference
// has no counterpart: its moments are the regressed spans as they come.
#include "common.h"

namespace {

constexpr int AC_THREADS = 1024;        // sixteen waves: wave w takes the lags of index w, w + 16, ...
constexpr int AC_TILE = 1024;           // frames of one pass: 16 per lane
constexpr int AC_HALO = 256;            // frames staged before the tile: the largest lag
constexpr int AC_MAX_LAG = 256;

constexpr int BT_THREADS = 1024;        // sixteen waves, a frame of a block per row of 16 lanes
constexpr int BT_ROWS = BT_THREADS / 16;
constexpr int BT_MAX_P = 256;
constexpr int BT_RING = 1024;           // >= dhi + dlo = 640 at P = 256: a block's writes never meet its reads
constexpr int BT_TILE = 1024;           // frames of the envelope staged at a time, two tiles in flight
constexpr int BT_PEN = 2 * BT_MAX_P - BT_MAX_P / 2 + 1;          // dhi - dlo + 1 at P = 256
constexpr int BT_CHAIN = 4096;          // beats of the backtrace kept in LDS (a longer chain is walked a second time)

__device__ __forceinline__ float quiet_nan() { return __uint_as_float(0x7FC00000u); }

// Maximum over each row of 16 lanes, on the DPP path (wave_max's first four steps): every lane ends with its row's value.  All 64
// lanes must be active.
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, dpp_f32<0xB1, 0xF>(v, v));                      // quad_perm [1,0,3,2]
    v = fmaxf(v, dpp_f32<0x4E, 0xF>(v, v));                      // quad_perm [2,3,0,1]
    v = fmaxf(v, dpp_f32<0x124, 0xF>(v, v));                     // row_ror:4
    v = fmaxf(v, dpp_f32<0x128, 0xF>(v, v));                     // row_ror:8
    return v;
}

// One workgroup per track.  The mean: thread i adds e[i], e[i + 1024], ... in ascending order, the 64 lanes of a wave by the DPP
// tree of wave_sum, the sixteen waves' totals one after the other from wave 0.  The sums: the track is walked in tiles of 1024 frames staged in
// LDS as x = e - m with the 256 frames before them; for one lag and one tile lane i adds the products of the frames f0 + i,
// f0 + i + 64, ... (16 terms, ascending), the lanes by the same tree, and the tile's total is added to the lag's running total
// (ascending tiles).  Frames outside [l, nf) add +0.  The order depends on nf alone.
__global__ __launch_bounds__(AC_THREADS) void tempo_autocorr_kernel(const float* env, int64_t env_ld, const int32_t* n_frames, int lag_min,
                                                                    int lag_max, const float* weight, float* ac, float* scale, int32_t* period) {
    __shared__ float sh[AC_HALO + AC_TILE];
    __shared__ float acc[AC_MAX_LAG + 1];
    __shared__ float score[AC_MAX_LAG];
    __shared__ float part[AC_THREADS / 64];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_lags = lag_max - lag_min + 1;
    const int64_t nf = n_frames[t];
    float* row = ac + t * (n_lags + 1);
    if (nf < 0 || nf > env_ld) {                                 // (uniform) a track that does not fit: no sums, no tempo
        for (int i = tid; i <= n_lags; i += AC_THREADS) row[i] = quiet_nan();
        if (tid == 0) {
            scale[t] = quiet_nan();
            period[t] = -1;
        }
        return;
    }
    const float* e = env + t * env_ld;
    float s = 0.f;
    for (int64_t f = tid; f < nf; f += AC_THREADS) s += e[f];
    s = wave_sum(s);
    if (lane == 0) part[wave] = s;
    for (int i = tid; i <= n_lags; i += AC_THREADS) acc[i] = 0.f;
    __syncthreads();
    float total = part[0];
    for (int w = 1; w < AC_THREADS / 64; ++w) total += part[w];
    const float m = total / (float)nf;
    for (int64_t f0 = 0; f0 < nf; f0 += AC_TILE) {
        __syncthreads();                                         // the pass before has read sh
        for (int i = tid; i < AC_HALO + AC_TILE; i += AC_THREADS) {
            const int64_t g = f0 - AC_HALO + i;
            sh[i] = (g >= 0 && g < nf) ? e[g] - m : 0.f;
        }
        __syncthreads();
        for (int idx = wave; idx <= n_lags; idx += AC_THREADS / 64) {            // index 0 is lag 0, index 1 + j lag lag_min + j
            const int l = idx == 0 ? 0 : lag_min + idx - 1;
            float p = 0.f;
#pragma unroll
            for (int i = 0; i < AC_TILE / 64; ++i) {
                const int c = AC_HALO + lane + 64 * i;
                const int64_t f = f0 + lane + 64 * i;
                const float prod = sh[c] * sh[c - l];
                p += (f >= l && f < nf) ? prod : 0.f;
            }
            p = wave_sum(p);
            if (lane == 0) acc[idx] += p;                        // a lag belongs to one wave: no other writer
        }
    }
    __syncthreads();
    for (int i = tid; i <= n_lags; i += AC_THREADS) row[i] = acc[i];
    const float ac0 = acc[0];
    if (tid < n_lags) score[tid] = (acc[1 + tid] / (float)(nf - (lag_min + tid))) * weight[tid];
    __syncthreads();
    if (tid == 0) {
        float best = 0.f;
        int p = -1;
        if (nf > lag_max && ac0 > 0.f)
            for (int j = 0; j < n_lags; ++j)
                if (score[j] > best) {                           // strict: of equal scores the smaller lag
                    best = score[j];
                    p = lag_min + j;
                }
        period[t] = p;
        scale[t] = p >= 0 ? 1.f / sqrtf(ac0 / (float)nf) : quiet_nan();
    }
}

// One workgroup per track.  Frame f reads cum of the frames f - dhi .. f - dlo only, so the dlo frames of a block are independent:
// a row of 16 lanes takes a frame, four frames a wave, the block's frames packed into as few waves as hold them.  (A wave per
// frame has the sixteen waves of the one CU issue two six-step 64-lane reductions for every frame, far more instructions than
// the frame's candidates need; a row reduces in four steps and one instruction serves four frames.)  A row's
// lanes take the candidates d = dlo + lane, + 16, ... (ascending, a strict > keeps the smaller d), and the row's argmax is two
// row_max: the value, then -(float)d among the lanes that hold it.  The order (value descending, d ascending) is strict over the
// candidates (a NaN sum is no candidate), so the result does not depend on the reduction's shape.
__global__ __launch_bounds__(BT_THREADS) void beat_track_kernel(const float* env, int64_t env_ld, const int32_t* n_frames, const int32_t* period,
                                                                const float* scale, float alpha, int64_t cap, float* time, int32_t* count,
                                                                float* cum, int32_t* back) {
    __shared__ float ring[BT_RING];                              // cum of the trailing frames, at f & (BT_RING - 1)
    __shared__ float loc[2 * BT_TILE];                           // e * scale of two tiles, at f & (2 BT_TILE - 1)
    __shared__ float pen[BT_PEN];
    __shared__ int32_t chain[BT_CHAIN];
    __shared__ int32_t chain_n;
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = tid & 15;
    const int64_t nf = n_frames[t];
    const int P = period[t];
    const float sc = scale[t];
    if (nf < 0 || nf > env_ld) {                                 // (every exit here is uniform)
        if (tid == 0) count[t] = -1;
        return;
    }
    if (P == -1) {                                               // no tempo: no beats
        if (tid == 0) count[t] = 0;
        return;
    }
    const int dlo = (P + 1) / 2, dhi = 2 * P;
    if (P < 2 || P > BT_MAX_P || !(fabsf(sc) < INFINITY) || (nf + dlo - 1) / dlo > cap) {
        if (tid == 0) count[t] = -1;
        return;
    }
    const float* e = env + t * env_ld;
    float* cu = cum + t * env_ld;
    int32_t* bk = back + t * env_ld;
    // (no loop vectorisation below: it pairs the products into packed-FP32 instructions, which this library keeps out -- see the Makefile)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = tid; i <= dhi - dlo; i += BT_THREADS) {
        const int d = dlo + i;
        pen[i] = -alpha * ((float)((d - P) * (d - P)) / (float)(d * P));
    }
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = tid; i < 2 * BT_TILE; i += BT_THREADS) loc[i] = i < nf ? e[i] * sc : 0.f;
    int64_t next = 2;                                            // (uniform) the tile staged next: tile k + 1 once a block starts in tile k
    __syncthreads();
    for (int64_t b0 = 0; b0 < nf; b0 += dlo) {
        if (b0 >= (next - 1) * BT_TILE) {                        // every frame of tile next - 2 is done: its half of loc is free, and no
            const int64_t f = next * BT_TILE + tid;              // frame of this block lies in tile next (2 dlo <= 256 frames ahead at most)
            loc[f & (2 * BT_TILE - 1)] = f < nf ? e[f] * sc : 0.f;
            ++next;
        }
        for (int i0 = 4 * wave; i0 < dlo && b0 + i0 < nf; i0 += BT_ROWS) {        // (uniform in the wave: the row reductions need every lane)
            const int64_t f = b0 + i0 + (lane >> 4);
            const bool mine = i0 + (lane >> 4) < dlo && f < nf;   // a row past the block or the track: no candidate, nothing written
            float bv = -INFINITY;
            int bd = 0;
            for (int d = dlo + l16; mine && d <= dhi && d <= f; d += 16) {
                const float v = ring[(f - d) & (BT_RING - 1)] + pen[d - dlo];
                if (v > bv) {
                    bv = v;
                    bd = d;
                }
            }
            const float best = row_max(bv);
            const float nd = row_max(bd > 0 && bv == best ? -(float)bd : -INFINITY);
            if (mine && l16 == 0) {
                const float lf = loc[f & (2 * BT_TILE - 1)];
                const bool link = best > 0.f;                    // -inf without a predecessor
                const float c = link ? lf + best : lf;
                ring[f & (BT_RING - 1)] = c;
                cu[f] = c;
                bk[f] = link ? (int32_t)(f - (int64_t)(-nd)) : -1;
            }
        }
        __syncthreads();
    }
    if (wave == 0) {                                             // the end frame: the argmax of cum over the last dhi frames, the earlier of equals
        float bv = -INFINITY;
        int64_t bf = -1;
        for (int64_t f = (nf > dhi ? nf - dhi : 0) + lane; f < nf; f += 64) {
            const float v = ring[f & (BT_RING - 1)];
            if (v > bv) {
                bv = v;
                bf = f;
            }
        }
        const float best = wave_max(bv);
        const float nfr = wave_max(bf >= 0 && bv == best ? -(float)bf : -INFINITY);
        if (lane == 0) {
            int32_t n = 0;
            for (int64_t f = nfr > -INFINITY ? (int64_t)(-nfr) : -1; f >= 0; f = bk[f]) {        // back[f] < f: the walk ends
                if (n < BT_CHAIN) chain[n] = (int32_t)f;
                ++n;
            }
            chain_n = n;
        }
    }
    __syncthreads();
    const int n = chain_n;                                       // <= ceil(nf / dlo) <= cap: two beats are dlo frames apart or more
    float* out = time + t * cap;
    for (int i = tid; i < n && i < BT_CHAIN; i += BT_THREADS) out[n - 1 - i] = (float)chain[i] * 0.01f;
    if (tid == 0) {
        if (n > BT_CHAIN) {
            int64_t f = chain[BT_CHAIN - 1];
            for (int i = BT_CHAIN; i < n; ++i) {
                f = bk[f];
                out[n - 1 - i] = (float)f * 0.01f;
            }
        }
        count[t] = n;
    }
}

}  // namespace

extern "C" int made_tempo_autocorr(const float* env, int64_t env_ld, const int32_t* n_frames, int64_t N, int32_t lag_min, int32_t lag_max,
                                   const float* weight, float* ac, float* scale, int32_t* period, void* stream) {
    MADE_REQUIRE(N >= 0 && env_ld >= 0, "made_tempo_autocorr: negative size");
    MADE_REQUIRE(lag_min >= 1 && lag_min <= lag_max && lag_max <= AC_MAX_LAG,
                 "made_tempo_autocorr: lags must satisfy 1 <= lag_min <= lag_max <= %d, got %d and %d", AC_MAX_LAG, (int)lag_min, (int)lag_max);
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && weight && ac && scale && period && (env || env_ld == 0), "made_tempo_autocorr: null pointer");
    MADE_REQUIRE(N < (1LL << 31) && env_ld < (1LL << 24), "made_tempo_autocorr: too many tracks or frames for one call");
    hipLaunchKernelGGL(tempo_autocorr_kernel, dim3((unsigned)N), dim3(AC_THREADS), 0, (hipStream_t)stream, env, env_ld, n_frames, (int)lag_min,
                       (int)lag_max, weight, ac, scale, period);
    return made_check_launch("made_tempo_autocorr");
}

extern "C" int made_beat_track(const float* env, int64_t env_ld, const int32_t* n_frames, const int32_t* period, const float* scale, int64_t N,
                               float alpha, int64_t cap, float* time, int32_t* count, float* cum, int32_t* back, void* stream) {
    MADE_REQUIRE(N >= 0 && env_ld >= 0 && cap >= 0, "made_beat_track: negative size");
    MADE_REQUIRE(alpha >= 0.f && alpha < INFINITY, "made_beat_track: alpha must be finite and >= 0");
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && period && scale && count && ((env && cum && back) || env_ld == 0) && (time || cap == 0),
                 "made_beat_track: null pointer");
    MADE_REQUIRE(N < (1LL << 31) && env_ld < (1LL << 24), "made_beat_track: too many tracks or frames for one call");
    const int64_t least = (env_ld + BT_MAX_P / 2 - 1) / (BT_MAX_P / 2);
    MADE_REQUIRE(cap >= least, "made_beat_track: cap must be >= ceil(env_ld / %d) = %lld (no period needs less), got %lld", BT_MAX_P / 2,
                 (long long)least, (long long)cap);
    hipLaunchKernelGGL(beat_track_kernel, dim3((unsigned)N), dim3(BT_THREADS), 0, (hipStream_t)stream, env, env_ld, n_frames, period, scale, alpha,
                       cap, time, count, cum, back);
    return made_check_launch("made_beat_track");
}
