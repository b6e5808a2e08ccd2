// Fitting: the last, optional step of grounding (mgsv_amd/grounding.py fit_grounding).  made_fit_moments gives every moment the
// length its video asks for, keeps it inside its track and moves its start onto the nearest onset of the track within a tolerance
// (the onset table: csrc/onsets.hip, mgsv_amd/onsets.py).  The reference returns the regressed span as it is.
// Compiled with -ffp-contract=off (csrc/Makefile): every step is one rounded f32 operation, so that the numpy f32 restatement
// (mgsv_amd/ops.py fit_moments_host, tests/fit_ref.py) is bit-exact.  min / max are the comparisons written out below, not fminf /
// fmaxf, so that a NaN and the zeros' signs go the same way in both.
#include "common.h"

namespace {

__device__ __forceinline__ float pick_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float pick_min(float a, float b) { return a < b ? a : b; }

__global__ __launch_bounds__(256) void fit_moments_kernel(const float* start, const float* end, const int32_t* track, const float* want,
                                                          int64_t E, const float* tlen, int64_t n_tracks, const int64_t* onset_start,
                                                          const float* onset_time, int64_t n_onsets, float tol, float* out_start,
                                                          float* out_end, float* shift, int32_t* onset) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float nan = __uint_as_float(0x7FC00000u);
    const int64_t tr = track[e];
    const float s0 = start[e], e0 = end[e];
    const float T = (tr >= 0 && tr < n_tracks) ? tlen[tr] : nan;
    if (s0 != s0 || e0 != e0 || T != T) {
        out_start[e] = nan;
        out_end[e] = nan;
        shift[e] = nan;
        onset[e] = -1;
        return;
    }
    const float w = want[e];
    float len = w == w ? w : e0 - s0;
    len = pick_min(pick_max(len, 0.f), T);
    const float c = 0.5f * (s0 + e0);
    const float last = T - len;                                  // the latest start that keeps the moment inside the track
    const float s1 = pick_min(pick_max(c - 0.5f * len, 0.f), last);
    float s2 = s1;
    int32_t which = -1;
    if (tol > 0.f && onset_start != nullptr && onset_time != nullptr) {
        int64_t a = onset_start[tr], b = onset_start[tr + 1];
        a = a < 0 ? 0 : (a > n_onsets ? n_onsets : a);
        b = b < a ? a : (b > n_onsets ? n_onsets : b);
        int64_t lo = a, hi = b;                                  // the first onset >= s1
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (onset_time[mid] < s1) lo = mid + 1;
            else hi = mid;
        }
        float best = 0.f;
        if (lo > a) {                                            // the last onset before s1
            const float o = onset_time[lo - 1];
            const float d = fabsf(o - s1);
            if (d <= tol && o <= last) {
                which = (int32_t)(lo - 1 - a);
                best = d;
                s2 = o;
            }
        }
        if (lo < b) {
            const float o = onset_time[lo];
            const float d = fabsf(o - s1);
            if (d <= tol && o <= last && (which < 0 || d < best)) {                  // (equal distances: the earlier stays)
                which = (int32_t)(lo - a);
                s2 = o;
            }
        }
    }
    out_start[e] = s2;
    out_end[e] = s2 + len;
    shift[e] = s2 - s0;
    onset[e] = which;
}

}  // namespace

extern "C" int made_fit_moments(const float* start, const float* end, const int32_t* track, const float* want, int64_t E,
                                const float* tlen, int64_t n_tracks, const int64_t* onset_start, const float* onset_time,
                                int64_t n_onsets, float tol, float* out_start, float* out_end, float* shift, int32_t* onset, void* stream) {
    MADE_REQUIRE(E >= 0 && E < (1LL << 31) && n_tracks >= 0 && n_tracks < (1LL << 31) && n_onsets >= 0,
                 "made_fit_moments: E and n_tracks must lie in [0, 2^31), n_onsets must be >= 0");
    MADE_REQUIRE(tol >= 0.f && tol < INFINITY, "made_fit_moments: tol must be finite and >= 0");
    if (E == 0) return MADE_OK;
    MADE_REQUIRE(start && end && track && want && (tlen || n_tracks == 0) && out_start && out_end && shift && onset,
                 "made_fit_moments: null pointer");
    MADE_REQUIRE(tol == 0.f || (onset_start && (onset_time || n_onsets == 0)), "made_fit_moments: tol > 0 needs the onset table");
    hipLaunchKernelGGL(fit_moments_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, (hipStream_t)stream, start, end, track, want, E,
                       tlen, n_tracks, onset_start, n_onsets ? onset_time : (const float*)nullptr, n_onsets, tol, out_start, out_end, shift,
                       onset);
    return made_check_launch("made_fit_moments");
}
