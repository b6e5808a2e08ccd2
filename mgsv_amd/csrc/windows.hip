// Windows: grounding in tracks longer than max_m_duration through overlapping windows (mgsv_amd/windows.py, grounding.py).  The
// unique AST feature rows spread over the windows that share them (made_gather_rows), the best w windows of every selected track
// (made_group_topw; made_group_topw_masked under made_eligibility's bits) and the windows' moments merged on the track's own time axis (made_merge_moments).  The reference has no
// counterpart: its dataset is cut to max_m_duration (dataloaders/dataloader_MGSV_EC_rawdata.py:95-158).
// Compiled with -ffp-contract=off (csrc/Makefile): made_merge_moments' f32 arithmetic is one rounding per operation, so that a
// numpy f32 restatement is bit-exact.
#include "common.h"

namespace {

constexpr int MERGE_MAX = 256;          // most candidates of one (video, track): w * Q

// One wave per destination row, 16-byte accesses.  An index outside [0, U) writes a zero row and reads nothing.
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* src, const int32_t* index, uint4* dst, int64_t U, int64_t R, int c16) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int lane = threadIdx.x & 63;
    const int64_t u = index[r];
    uint4* d = dst + r * c16;
    if (u >= 0 && u < U) {
        const uint4* s = src + u * c16;
        for (int i = lane; i < c16; i += 64) d[i] = s[i];
    } else {
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (int i = lane; i < c16; i += 64) d[i] = z;
    }
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor((unsigned long long)v, o);
        v = y > v ? y : v;
    }
    return v;
}

// One wave per (video, selected group): w rounds, each taking the largest (score key, lowest column) of the group's members that
// lies strictly below the previous round's pick -- the members come from the CSR, the row is never scanned.  MASKED: a member whose
// bit of mask [row, mask_ld words] (made_eligibility's layout) is clear is skipped: it fills no slot.
template <bool MASKED>
__global__ __launch_bounds__(256) void group_topw_kernel(const float* sims, int64_t ld, const uint32_t* mask, int64_t mask_ld,
                                                         const int32_t* sel, const int32_t* col_group,
                                                         const int32_t* start, const int32_t* cols, int n_cols, int64_t NK, int K, int Nm,
                                                         int G, int w, int32_t* idx_out, float* score_out) {
    const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= NK) return;
    const int lane = threadIdx.x & 63;
    const float* s = sims + (e / K) * ld;
    const uint32_t* mb = MASKED ? mask + (e / K) * mask_ld : nullptr;
    const int c0 = sel[e];
    int a = 0, b = 0;
    if (c0 >= 0 && c0 < Nm) {
        const int g = col_group[c0];
        if ((unsigned)g < (unsigned)G) {
            a = min(max(start[g], 0), n_cols);
            b = min(max(start[g + 1], a), n_cols);
        }
    }
    uint64_t bound = ~0ull;                                      // picks so far are >= bound
    for (int j = 0; j < w; ++j) {
        uint64_t best = 0ull;                                    // (every member's value is > 0: score keys are >= 1)
        for (int i = a + lane; i < b; i += 64) {
            const int c = cols[i];
            if ((unsigned)c >= (unsigned)Nm) continue;
            if constexpr (MASKED) {
                if (!((mb[c >> 5] >> (c & 31)) & 1u)) continue;
            }
            const uint64_t v = ((uint64_t)score_key(s[c]) << 32) | (uint32_t)(0x7FFFFFFF - c);
            if (v < bound && v > best) best = v;
        }
        best = wave_max_u64(best);
        if (lane == 0) {
            idx_out[e * w + j] = best ? 0x7FFFFFFF - (int)(uint32_t)best : -1;
            score_out[e * w + j] = key_score((uint32_t)(best >> 32));
        }
        bound = best;                                            // (0 after the group's last member: nothing passes any more)
    }
}

struct MergeShared {
    uint64_t a[MERGE_MAX];               // (window similarity key, foreground probability key): descending
    uint64_t b[MERGE_MAX];               // (column, query): ascending
    float s[MERGE_MAX], e[MERGE_MAX], conf[MERGE_MAX];          // sorted candidates: absolute start / end, confidence
    int col[MERGE_MAX];
    int dropped[MERGE_MAX];
};

// One wave per (video, track).  cand [P, w, Q, 3] = (start, end, foreground probability) of every query of the track's w windows,
// seconds on the window's own axis, unclamped.  Rank sort by the total order, then the greedy walk.
__global__ __launch_bounds__(64) void merge_moments_kernel(const float* cand, const int32_t* win_col, const float* win_score,
                                                           const float* offset, const float* duration, int Nm, int w, int Q,
                                                           int use_prob, float max_m_duration, float nms_iou, int n, float* start_out,
                                                           float* end_out, float* conf_out, int32_t* window_out) {
    __shared__ MergeShared sh;
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    const int M = w * Q;
    int Mv = 0;                                                  // candidates of the windows that are there (uniform)
    for (int j = 0; j < w; ++j) {
        const int c = win_col[p * w + j];
        Mv += (c >= 0 && c < Nm) ? Q : 0;
    }
    for (int i = lane; i < M; i += 64) {
        const int j = i / Q, q = i % Q;
        const int c = win_col[p * w + j];
        const bool ok = c >= 0 && c < Nm;
        uint64_t a = 0ull;                                       // (a window that is not there: after every candidate)
        if (ok) {
            const uint32_t kp = use_prob ? score_key(cand[((p * w + j) * Q + q) * 3 + 2]) : 0u;
            a = ((uint64_t)score_key(win_score[p * w + j]) << 32) | kp;
        }
        sh.a[i] = a;
        sh.b[i] = ((uint64_t)(uint32_t)(ok ? c : 0x7FFFFFFF) << 32) | (uint32_t)i;      // (i ascends with the query inside a window)
    }
    __syncthreads();
    for (int i = lane; i < M; i += 64) {
        const uint64_t a = sh.a[i], b = sh.b[i];
        int r = 0;
        for (int t = 0; t < M; ++t) {
            const uint64_t at = sh.a[t], bt = sh.b[t];
            r += (at > a || (at == a && bt < b)) ? 1 : 0;
        }
        if (a != 0ull) {
            const int j = i / Q;
            const int c = win_col[p * w + j];
            const float* x = cand + ((p * w + j) * Q + i % Q) * 3;
            float hi = max_m_duration;
            if (duration) hi = fminf(hi, duration[c]);
            const float off = offset[c];
            sh.s[r] = fminf(fmaxf(x[0], 0.f), hi) + off;
            sh.e[r] = fminf(fmaxf(x[1], 0.f), hi) + off;
            sh.conf[r] = use_prob ? x[2] : __uint_as_float(0x7FC00000u);
            sh.col[r] = c;
        }
        sh.dropped[i] = 0;
    }
    __syncthreads();
    int kept = 0;
    for (int i = 0; i < Mv && kept < n; ++i) {                   // (uniform: dropped[] is read after the barrier that ends each step)
        if (sh.dropped[i]) continue;
        const float s1 = sh.s[i], e1 = sh.e[i];
        if (lane == 0) {
            start_out[p * n + kept] = s1;
            end_out[p * n + kept] = e1;
            conf_out[p * n + kept] = sh.conf[i];
            window_out[p * n + kept] = sh.col[i];
        }
        ++kept;
        for (int t = i + 1 + lane; t < Mv; t += 64) {
            if (sh.dropped[t]) continue;
            const float s2 = sh.s[t], e2 = sh.e[t];
            const float inter = fmaxf(0.f, fminf(e1, e2) - fmaxf(s1, s2));
            const float uni = (e1 - s1) + (e2 - s2) - inter;
            const float iou = uni > 0.f ? inter / uni : 0.f;
            if (iou > nms_iou) sh.dropped[t] = 1;
        }
        __syncthreads();
    }
    for (int t = kept + lane; t < n; t += 64) {
        const float nan = __uint_as_float(0x7FC00000u);
        start_out[p * n + t] = nan;
        end_out[p * n + t] = nan;
        conf_out[p * n + t] = nan;
        window_out[p * n + t] = -1;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int made_gather_rows(const void* src, int64_t U, const int32_t* index, int64_t R, int64_t C, void* dst, int32_t dtype,
                                void* stream) {
    MADE_REQUIRE(index && dst && (src || U == 0), "made_gather_rows: null pointer");
    MADE_REQUIRE(dtype == MADE_F32 || dtype == MADE_BF16, "made_gather_rows: dtype must be MADE_F32 or MADE_BF16");
    MADE_REQUIRE(U >= 0 && R >= 0 && C >= 1 && R < (1LL << 32), "made_gather_rows: bad dims");
    const int64_t esz = dtype == MADE_F32 ? 4 : 2;
    MADE_REQUIRE((C * esz) % 16 == 0 && C * esz / 16 < (1LL << 31) && aligned16(src) && aligned16(dst),
                 "made_gather_rows: rows must be 16-byte aligned (C * element size a multiple of 16)");
    if (R == 0) return MADE_OK;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, index,
                       (uint4*)dst, U, R, (int)(C * esz / 16));
    return made_check_launch("made_gather_rows");
}

namespace {

template <bool MASKED>
int group_topw_launch(const float* sims, int64_t ld, const uint32_t* bits, int64_t bits_ld, const int32_t* sel, const int32_t* col_group,
                      const int32_t* start, const int32_t* cols, int64_t n_cols, int64_t Nv, int64_t Nm, int64_t n_groups, int64_t K,
                      int64_t w, int32_t* idx_out, float* score_out, void* stream) {
    MADE_REQUIRE(sims && sel && col_group && start && cols && idx_out && score_out, "made_group_topw: null pointer");
    MADE_REQUIRE(Nv >= 0 && Nm > 0 && ld >= Nm && Nm < (1LL << 31), "made_group_topw: bad dims (Nv >= 0, Nm > 0, ld >= Nm)");
    MADE_REQUIRE(K >= 1 && n_groups >= 1 && n_groups < (1LL << 31) && n_cols >= 0 && n_cols < (1LL << 31), "made_group_topw: bad dims");
    MADE_REQUIRE(w >= 1 && w <= 16, "made_group_topw: w must lie in [1, 16]");
    MADE_REQUIRE(Nv * K < (1LL << 32), "made_group_topw: too many (video, group) entries");
    if (MASKED) MADE_REQUIRE(bits_ld >= (Nm + 31) / 32, "made_group_topw_masked: bits_ld must be >= ceil(Nm / 32) words");
    if (Nv == 0) return MADE_OK;
    hipLaunchKernelGGL(group_topw_kernel<MASKED>, dim3((unsigned)((Nv * K + 3) / 4)), dim3(256), 0, (hipStream_t)stream, sims, ld, bits,
                       bits_ld, sel, col_group, start, cols, (int)n_cols, Nv * K, (int)K, (int)Nm, (int)n_groups, (int)w, idx_out, score_out);
    return made_check_launch("made_group_topw");
}

}  // namespace

extern "C" int made_group_topw(const float* sims, int64_t ld, const int32_t* sel, const int32_t* col_group, const int32_t* start,
                               const int32_t* cols, int64_t n_cols, int64_t Nv, int64_t Nm, int64_t n_groups, int64_t K, int64_t w,
                               int32_t* idx_out, float* score_out, void* stream) {
    return group_topw_launch<false>(sims, ld, nullptr, 0, sel, col_group, start, cols, n_cols, Nv, Nm, n_groups, K, w, idx_out, score_out, stream);
}

extern "C" int made_group_topw_masked(const float* sims, int64_t ld, const uint32_t* bits, int64_t bits_ld, const int32_t* sel,
                                      const int32_t* col_group, const int32_t* start, const int32_t* cols, int64_t n_cols, int64_t Nv,
                                      int64_t Nm, int64_t n_groups, int64_t K, int64_t w, int32_t* idx_out, float* score_out, void* stream) {
    if (!bits) return group_topw_launch<false>(sims, ld, nullptr, 0, sel, col_group, start, cols, n_cols, Nv, Nm, n_groups, K, w, idx_out, score_out, stream);
    return group_topw_launch<true>(sims, ld, bits, bits_ld, sel, col_group, start, cols, n_cols, Nv, Nm, n_groups, K, w, idx_out, score_out, stream);
}

extern "C" int made_merge_moments(const float* cand, const int32_t* win_col, const float* win_score, const float* offset,
                                  const float* duration, int64_t P, int64_t Nm, int64_t w, int64_t Q, int32_t use_prob,
                                  float max_m_duration, float nms_iou, int64_t n, float* start_out, float* end_out, float* conf_out,
                                  int32_t* window_out, void* stream) {
    MADE_REQUIRE(cand && win_col && win_score && offset && start_out && end_out && conf_out && window_out, "made_merge_moments: null pointer");
    MADE_REQUIRE(P >= 0 && P < (1LL << 31) && Nm >= 0 && Nm < (1LL << 31) && w >= 1 && Q >= 1 && n >= 1 && n < (1LL << 31),
                 "made_merge_moments: bad dims");
    MADE_REQUIRE(nms_iou >= 0.f, "made_merge_moments: nms_iou must be >= 0");
    MADE_UNSUPPORTED(w * Q <= MERGE_MAX && w <= MERGE_MAX && Q <= MERGE_MAX, "made_merge_moments: at most %d candidates per (video, track), got w * Q = %lld",
                     MERGE_MAX, (long long)(w * Q));
    if (P == 0) return MADE_OK;
    hipLaunchKernelGGL(merge_moments_kernel, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, cand, win_col, win_score, offset, duration,
                       (int)Nm, (int)w, (int)Q, (int)(use_prob != 0), max_m_duration, nms_iou, (int)n, start_out, end_out, conf_out, window_out);
    return made_check_launch("made_merge_moments");
}
