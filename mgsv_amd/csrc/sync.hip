// Cut sync: fitting a moment so that the video's cuts land on the track's attacks (mgsv_amd/grounding.py fit_grounding with
// Fit.cuts).  made_sync_moments evaluates the rule include/made_hip.h states: the candidates are the unsnapped start and every
// start that puts an anchor (the video's beginning or one of its cuts) on an onset within `snap`; each is scored by how many
// anchors fall near an onset, and the best under a strict order wins.  made_fit_moments (csrc/fit.hip) is the special case of a
// video without cuts, and its front (len, c, last, s1) is restated here operation for operation.
// Compiled with -ffp-contract=off (csrc/Makefile): every step is one rounded f32 operation, so that the numpy f32 restatement
// (mgsv_amd/ops.py sync_moments_host, tests/sync_ref.py) is bit-exact.  min / max are the comparisons written out, not fminf / fmaxf.
//
// One wave per entry, four entries per workgroup.  Lane j < |A| owns anchor j: it finds the contiguous range of onsets its anchor
// admits by two binary searches; a wave prefix sum numbers the candidates.  Every lane then takes candidates lane, lane + 64, ...,
// scores each over all anchors and keeps its best; a butterfly with the same strict comparator reduces the 64 bests.  The anchors
// and the prefix sit in LDS (776 bytes per wave); no atomics, no workspace, no scratch.
#include "common.h"

namespace {

constexpr int SYNC_WAVES = 4;                                      // entries per workgroup
constexpr int SYNC_MAX_CUTS = 63;                                  // cuts read of a video's row: |A| <= 64, one anchor per lane

__device__ __forceinline__ float pick_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float pick_min(float a, float b) { return a < b ? a : b; }

struct SyncCand {
    float sync, dist, s;
    int32_t j, i, hits;                                            // j: the anchor (INT32_MAX: the unsnapped start), i: the onset inside the track
};

// the strict order of the contract: larger sync, smaller |s - s1|, smaller s, smaller anchor, smaller onset
__device__ __forceinline__ bool sync_better(const SyncCand& x, const SyncCand& y) {
    if (x.sync != y.sync) return x.sync > y.sync;
    if (x.dist != y.dist) return x.dist < y.dist;
    if (x.s != y.s) return x.s < y.s;
    if (x.j != y.j) return x.j < y.j;
    return x.i < y.i;
}

__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void sync_moments_kernel(const float* start, const float* end, const int32_t* track, const int32_t* video,
                                                           const float* want, int64_t E, const float* tlen, int64_t n_tracks,
                                                           const int64_t* onset_start, const float* onset_time, int64_t n_onsets,
                                                           const int64_t* cut_start, const float* cut_time, int64_t n_videos, int64_t n_cuts,
                                                           float snap, float cut_tol, float* out_start, float* out_end, float* shift,
                                                           int32_t* onset, int32_t* anchor, float* sync, int32_t* hits) {
    __shared__ float s_anchor[SYNC_WAVES][WAVE];
    __shared__ int64_t s_pre[SYNC_WAVES][WAVE + 1];                // s_pre[w][j]: the number of candidates of the anchors before j
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * SYNC_WAVES + w;
    const float nan = __uint_as_float(0x7FC00000u);
    float* const A = s_anchor[w];
    int64_t* const pre = s_pre[w];

    // ---- the front, made_fit_moments' (every lane of the wave computes the same values)
    bool live = e < E;
    float s0 = 0.f, len = 0.f, last = 0.f, s1 = 0.f;
    int64_t oa = 0, ob = 0;                                        // the track's onsets: onset_time[oa .. ob)
    if (live) {
        const int64_t tr = track[e];
        s0 = start[e];
        const float e0 = end[e];
        const float T = (tr >= 0 && tr < n_tracks) ? tlen[tr] : nan;
        if (s0 != s0 || e0 != e0 || T != T) {
            if (lane == 0) {
                out_start[e] = nan;
                out_end[e] = nan;
                shift[e] = nan;
                sync[e] = nan;
                onset[e] = -1;
                anchor[e] = -1;
                hits[e] = -1;
            }
            live = false;
        } else {
            const float wn = want[e];
            len = wn == wn ? wn : e0 - s0;
            len = pick_min(pick_max(len, 0.f), T);
            const float c = 0.5f * (s0 + e0);
            last = T - len;
            s1 = pick_min(pick_max(c - 0.5f * len, 0.f), last);
            oa = clamp_index(onset_start[tr], 0, n_onsets);
            ob = clamp_index(onset_start[tr + 1], oa, n_onsets);
        }
    }

    // ---- anchors: 0, then the cuts inside (0, len), compacted in order
    int nA = 1;
    if (live) {
        const int64_t vd = video[e];
        int64_t ca = 0, cb = 0;
        if (vd >= 0 && vd < n_videos) {
            ca = clamp_index(cut_start[vd], 0, n_cuts);
            cb = clamp_index(cut_start[vd + 1], ca, n_cuts);
            if (cb - ca > SYNC_MAX_CUTS) cb = ca + SYNC_MAX_CUTS;
        }
        float c = 0.f;
        bool keep = false;
        if (lane < cb - ca) {
            c = cut_time[ca + lane];
            keep = c > 0.f && c < len;
        }
        const unsigned long long m = __ballot(keep);
        nA = 1 + __popcll(m);
        if (lane == 0) A[0] = 0.f;
        if (keep) A[1 + __popcll(m & ((1ull << lane) - 1ull))] = c;
    }
    __syncthreads();

    // ---- lane j: the onsets anchor j admits, [lo, lo + cnt): s = o - a with |s - s1| <= snap, s >= 0, s <= last.  s is monotone
    // in o, so "s - s1 >= -snap and s >= 0" holds from some onset on and "s - s1 <= snap and s <= last" up to some onset.
    int64_t lo = 0, cnt = 0;
    if (live && lane < nA) {
        const float a = A[lane];
        int64_t l = oa, h = ob;                                    // the first onset that is not too early
        while (l < h) {
            const int64_t mid = l + ((h - l) >> 1);
            const float s = onset_time[mid] - a;
            if (s - s1 >= -snap && s >= 0.f) h = mid;
            else l = mid + 1;
        }
        lo = l;
        h = ob;                                                    // the first onset that is too late
        l = oa;
        while (l < h) {
            const int64_t mid = l + ((h - l) >> 1);
            const float s = onset_time[mid] - a;
            if (s - s1 <= snap && s <= last) l = mid + 1;
            else h = mid;
        }
        cnt = l > lo ? l - lo : 0;
    }
    int64_t incl = cnt;                                            // inclusive prefix sum over the lanes
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int64_t up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const int64_t N = __shfl(incl, WAVE - 1);                      // lanes >= nA hold no candidates
    if (live) {
        if (lane < nA) pre[lane] = incl - cnt;
        if (lane == nA - 1) pre[nA] = incl;
    }
    __syncthreads();
    if (!live) return;

    // ---- candidates: number 0 is the unsnapped start, number 1 + pre[j] + r is onset lo_j + r under anchor j
    const float inf = __uint_as_float(0x7F800000u);
    SyncCand best = {-inf, 0.f, 0.f, 0, 0, 0};                      // (a lane without candidates: loses to every real one, sync >= 0)
    for (int64_t q0 = 0; q0 <= N; q0 += WAVE) {
        const int64_t q = q0 + lane;
        const bool has = q <= N;
        const bool snapped = has && q > 0;
        int j = 0;
        if (snapped) {                                             // the last anchor with pre[j] <= q - 1 (anchors without candidates are passed over)
            int l = 0, h = nA - 1;
            while (l < h) {
                const int mid = (l + h + 1) >> 1;
                if (pre[mid] <= q - 1) l = mid;
                else h = mid - 1;
            }
            j = l;
        }
        const int64_t lo_j = __shfl(lo, j);
        SyncCand c = {0.f, 0.f, s1, 0x7FFFFFFF, -1, 0};
        if (snapped) {
            const int64_t i = lo_j + (q - 1 - pre[j]);
            c.s = onset_time[i] - A[j];
            c.dist = fabsf(c.s - s1);
            c.j = j;
            c.i = (int32_t)(i - oa);
        }
        if (has) {
            for (int k = 0; k < nA; ++k) {                          // the score: every anchor's distance to the nearest onset
                const float p = c.s + A[k];
                int64_t l = oa, h = ob;                            // the first onset >= p
                while (l < h) {
                    const int64_t mid = l + ((h - l) >> 1);
                    if (onset_time[mid] < p) l = mid + 1;
                    else h = mid;
                }
                float d = inf;
                if (l > oa) d = p - onset_time[l - 1];
                if (l < ob) {
                    const float dr = onset_time[l] - p;
                    d = dr < d ? dr : d;
                }
                const bool hit = d <= cut_tol;
                const float t = hit ? 1.f - d / cut_tol : 0.f;
                c.sync = c.sync + t;
                c.hits += hit ? 1 : 0;
            }
            if (sync_better(c, best)) best = c;
        }
    }

    // ---- the wave's best: the order is strict, so every lane ends with the same candidate whatever the shape of the reduction
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        SyncCand x;
        x.sync = __shfl_xor(best.sync, o);
        x.dist = __shfl_xor(best.dist, o);
        x.s = __shfl_xor(best.s, o);
        x.j = __shfl_xor(best.j, o);
        x.i = __shfl_xor(best.i, o);
        x.hits = __shfl_xor(best.hits, o);
        if (sync_better(x, best)) best = x;
    }
    if (lane == 0) {
        out_start[e] = best.s;
        out_end[e] = best.s + len;
        shift[e] = best.s - s0;
        onset[e] = best.i;
        anchor[e] = best.j == 0x7FFFFFFF ? -1 : best.j;
        sync[e] = best.sync;
        hits[e] = best.hits;
    }
}

}  // namespace

extern "C" int made_sync_moments(const float* start, const float* end, const int32_t* track, const int32_t* video, const float* want,
                                 int64_t E, const float* tlen, int64_t n_tracks, const int64_t* onset_start, const float* onset_time,
                                 int64_t n_onsets, const int64_t* cut_start, const float* cut_time, int64_t n_videos, int64_t n_cuts,
                                 float snap, float cut_tol, float* out_start, float* out_end, float* shift, int32_t* onset, int32_t* anchor,
                                 float* sync, int32_t* hits, void* stream) {
    MADE_REQUIRE(E >= 0 && E < (1LL << 31) && n_tracks >= 0 && n_tracks < (1LL << 31) && n_videos >= 0 && n_videos < (1LL << 31),
                 "made_sync_moments: E, n_tracks and n_videos must lie in [0, 2^31)");
    MADE_REQUIRE(n_onsets >= 0 && n_cuts >= 0, "made_sync_moments: n_onsets and n_cuts must be >= 0");
    MADE_REQUIRE(snap > 0.f && snap < INFINITY, "made_sync_moments: snap must be finite and > 0");
    MADE_REQUIRE(cut_tol > 0.f && cut_tol < INFINITY, "made_sync_moments: cut_tol must be finite and > 0");
    if (E == 0) return MADE_OK;
    MADE_REQUIRE(start && end && track && video && want && (tlen || n_tracks == 0) && out_start && out_end && shift && onset && anchor &&
                     sync && hits,
                 "made_sync_moments: null pointer");
    MADE_REQUIRE((onset_start || n_tracks == 0) && (onset_time || n_onsets == 0), "made_sync_moments: the onset table is needed");
    MADE_REQUIRE((cut_start || n_videos == 0) && (cut_time || n_cuts == 0), "made_sync_moments: the cut table is needed");
    hipLaunchKernelGGL(sync_moments_kernel, dim3((unsigned)((E + SYNC_WAVES - 1) / SYNC_WAVES)), dim3(256), 0, (hipStream_t)stream, start,
                       end, track, video, want, E, tlen, n_tracks, onset_start, onset_time, n_onsets, cut_start, cut_time, n_videos, n_cuts,
                       snap, cut_tol, out_start, out_end, shift, onset, anchor, sync, hits);
    return made_check_launch("made_sync_moments");
}
