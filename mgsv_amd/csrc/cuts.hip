// Cuts: where a video's shots change, from its decoded frames (mgsv_amd/cuts.py).  made_frame_hist reduces every frame to a 4 KB
// signature (a 64-bin luma histogram in each cell of a 4 x 4 grid), made_hist_distance is the L1 distance of neighbouring
// signatures, made_cut_peaks picks its local maxima that stand out of their surroundings.  Integer arithmetic from the first byte to
// the last comparison: no order of additions can change a bit.  The reference has no counterpart: its videos come as features.
#include "common.h"

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_BINS = 1024;           // 16 cells x 64 luma bins
constexpr int STEP_PIXELS = 16;           // pixels of one lane-step: 48 bytes, three 16-byte loads
constexpr int CHUNK_STEPS = 4;            // lane-steps a thread takes of one chunk
constexpr int CHUNK_PIXELS = HIST_THREADS * STEP_PIXELS * CHUNK_STEPS;       // 16 384 pixels (48 KB) a workgroup takes at a time
constexpr int MAX_PIXELS = 1 << 24;

constexpr int PEAK_TILE = 1024;           // frames one pass of a workgroup decides
constexpr int PEAK_HALO = 128;            // frames staged on either side: the largest w_avg (w_max is smaller)
constexpr int PEAK_THREADS = 256;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROW_MASK, 0xF, false);
}

// common.h wave_sum on integers: the total of the 64 lanes, the same value in every lane.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    v += dpp_u32<0xB1, 0xF>(v, v);                               // quad_perm [1,0,3,2]
    v += dpp_u32<0x4E, 0xF>(v, v);                               // quad_perm [2,3,0,1]
    v += dpp_u32<0x124, 0xF>(v, v);                              // row_ror:4
    v += dpp_u32<0x128, 0xF>(v, v);                              // row_ror:8
    v += dpp_u32<0x142, 0xA>(0u, v);                             // row_bcast:15 -> rows 1, 3
    v += dpp_u32<0x143, 0xC>(0u, v);                             // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

struct Step { uint32_t w[12]; };         // 48 bytes = 16 RGB pixels, little-endian words

__device__ __forceinline__ uint32_t step_byte(const Step& s, int i) { return (s.w[i >> 2] >> ((i & 3) * 8)) & 255u; }

// the 4 x 4 grid of a frame: cell column = 4 c / W = the number of k in 1 .. 3 with c >= ceil(k W / 4); rows alike
struct Grid { int cb1, cb2, cb3, rb1, rb2, rb3, W; };

__device__ __forceinline__ int cell_of(const Grid& g, int r, int c) {
    return 4 * ((r >= g.rb1) + (r >= g.rb2) + (r >= g.rb3)) + (c >= g.cb1) + (c >= g.cb2) + (c >= g.cb3);
}

// The first nv of the 16 pixels of `s`, the first one at (r, c), into the wave's histogram h.  MERGE: a run of equal (cell, bin) is
// one LDS add of its length (false: the measurement variant, an add per pixel).  WIDE (W >= 64, so every cell is 16 columns wide or
// more): the 16 pixels change their cell once at most -- at a cell boundary or at the end of the row -- jb pixels in; otherwise
// (r, c) is carried along, an increment with wrap, and every pixel looks its cell up.
template <bool MERGE, bool WIDE>
__device__ __forceinline__ void count_step(uint32_t* h, const Step& s, int nv, int r, int c, const Grid& g) {
    const int cell_a = cell_of(g, r, c);
    int cell_b = cell_a, jb = STEP_PIXELS;
    if (WIDE) {
        const int nb = c < g.cb1 ? g.cb1 : c < g.cb2 ? g.cb2 : c < g.cb3 ? g.cb3 : g.W;
        jb = nb - c;
        cell_b = nb == g.W ? cell_of(g, r + 1, 0) : cell_a + 1;
    }
    int cur = 0;
    uint32_t run = 0u;
#pragma unroll
    for (int j = 0; j < STEP_PIXELS; ++j) {
        const uint32_t R = step_byte(s, 3 * j), G = step_byte(s, 3 * j + 1), B = step_byte(s, 3 * j + 2);
        const uint32_t Y = (77u * R + 150u * G + 29u * B + 128u) >> 8;
        int cell;
        if (WIDE) {
            cell = j < jb ? cell_a : cell_b;
        } else {
            cell = cell_of(g, r, c);
            if (++c == g.W) { c = 0; ++r; }
        }
        const int key = cell * 64 + (int)(Y >> 2);
        const bool valid = j < nv;
        if (valid && run > 0u && (!MERGE || key != cur)) {
            atomicAdd(&h[cur], run);
            run = 0u;
        }
        if (valid) { cur = key; run += 1u; }
    }
    if (run > 0u) atomicAdd(&h[cur], run);
}

// One workgroup takes the chunks g, g + per_frame, ... of frame blockIdx.x / per_frame: a chunk is 16 384 consecutive pixels, a
// lane-step 16 of them (48 bytes, so every step of a frame has the alignment of the frame's first byte: three 16-byte loads, or
// twelve dword loads, or byte loads -- the frame's last, partial step always by bytes, never past the frame).  All paths fill the
// same 12 words.  MERGE false: the measurement variant without the run merging (tools/cuts_bench.py; the same counts).
template <bool MERGE>
__global__ __launch_bounds__(HIST_THREADS) void frame_hist_kernel(const uint8_t* frames, int64_t frames_len, const MadeCutFrameDesc* desc,
                                                                  int per_frame, uint32_t* hist) {
    __shared__ uint32_t sh[HIST_WAVES][HIST_BINS];
    const int64_t f = blockIdx.x / per_frame;
    const int g = blockIdx.x % per_frame;
    const int tid = threadIdx.x, wave = tid >> 6;
    const MadeCutFrameDesc d = desc[f];
    const int64_t P = (int64_t)d.H * d.W;
    // (uniform) a descriptor out of range or past the buffer: the frame's counts stay zero
    if (d.H < 1 || d.W < 1 || P > MAX_PIXELS || d.offset < 0 || d.offset > frames_len || 3 * P > frames_len - d.offset) return;
    if ((int64_t)g * CHUNK_PIXELS >= P) return;                  // (uniform) no chunk for this workgroup
    for (int b = tid; b < HIST_WAVES * HIST_BINS; b += HIST_THREADS) (&sh[0][0])[b] = 0u;
    __syncthreads();
    uint32_t* h = sh[wave];
    const uint8_t* base = frames + d.offset;
    const int align = ((uintptr_t)base & 15u) == 0 ? 16 : ((uintptr_t)base & 3u) == 0 ? 4 : 1;        // (uniform)
    const int H = d.H, W = d.W, n_px = (int)P;
    const Grid grid = {(W + 3) >> 2, (2 * W + 3) >> 2, (3 * W + 3) >> 2, (H + 3) >> 2, (2 * H + 3) >> 2, (3 * H + 3) >> 2, W};
    for (int64_t c0 = (int64_t)g * CHUNK_PIXELS; c0 < P; c0 += (int64_t)per_frame * CHUNK_PIXELS) {
        for (int it = 0; it < CHUNK_STEPS; ++it) {
            const int p0 = (int)c0 + (it * HIST_THREADS + tid) * STEP_PIXELS;
            const int nv = p0 >= n_px ? 0 : (n_px - p0 < STEP_PIXELS ? n_px - p0 : STEP_PIXELS);
            Step s;
#pragma unroll
            for (int i = 0; i < 12; ++i) s.w[i] = 0u;
            const uint8_t* src = base + 3 * (int64_t)p0;
            if (nv == STEP_PIXELS && align == 16) {
                const uint4* q = (const uint4*)src;
                const uint4 a = q[0], b = q[1], c = q[2];
                s.w[0] = a.x; s.w[1] = a.y; s.w[2] = a.z; s.w[3] = a.w;
                s.w[4] = b.x; s.w[5] = b.y; s.w[6] = b.z; s.w[7] = b.w;
                s.w[8] = c.x; s.w[9] = c.y; s.w[10] = c.z; s.w[11] = c.w;
            } else if (nv == STEP_PIXELS && align == 4) {
                const uint32_t* q = (const uint32_t*)src;
#pragma unroll
                for (int i = 0; i < 12; ++i) s.w[i] = q[i];
            } else if (nv > 0) {
#pragma unroll
                for (int i = 0; i < 48; ++i)
                    if (i < 3 * nv) s.w[i >> 2] |= (uint32_t)src[i] << ((i & 3) * 8);
            }
            int r = 0, c = 0;
            if (nv > 0) { r = p0 / W; c = p0 - r * W; }          // the one division of the step
            if (W >= 4 * STEP_PIXELS) count_step<MERGE, true>(h, s, nv, r, c, grid);         // (uniform)
            else count_step<MERGE, false>(h, s, nv, r, c, grid);
        }
    }
    __syncthreads();
    uint32_t* out = hist + f * HIST_BINS;
    for (int b = tid; b < HIST_BINS; b += HIST_THREADS) {
        uint32_t t = 0u;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) t += sh[w][b];
        if (t) atomicAdd(&out[b], t);                            // integer adds into the zeroed signature: any order, the same bits
    }
}

// One wave per frame, four frames per workgroup: lane l reads words 16 l .. 16 l + 15 of both signatures (four 16-byte loads each).
__global__ __launch_bounds__(256) void hist_distance_kernel(const uint4* hist, const uint8_t* first_of_video, int64_t n_frames, uint32_t* D) {
    const int64_t f = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= n_frames) return;                                   // (uniform in the wave)
    uint32_t v = 0u;
    if (f > 0 && first_of_video[f] == 0) {                       // (uniform in the wave)
        const uint4* a = hist + f * (HIST_BINS / 4);
        const uint4* b = a - HIST_BINS / 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 x = a[q * 64 + lane], y = b[q * 64 + lane];
            v += (x.x > y.x ? x.x - y.x : y.x - x.x) + (x.y > y.y ? x.y - y.y : y.y - x.y) + (x.z > y.z ? x.z - y.z : y.z - x.z) +
                 (x.w > y.w ? x.w - y.w : y.w - x.w);
        }
    }
    v = wave_sum_u32(v);
    if (lane == 0) D[f] = v;
}

// made_onset_peaks' walk (onsets.hip) on integers: one workgroup per video, a pass stages frames [f0 - 128, f0 + 1024 + 128) of the
// video's distances, every thread decides frames f0 + 256 j + tid for j < 4, and each j is compacted in frame order.
__global__ __launch_bounds__(PEAK_THREADS) void cut_peaks_kernel(const uint32_t* D, int64_t D_ld, const int32_t* n_frames, const uint32_t* thr,
                                                                 int w_max, int w_avg, int ratio_q8, int64_t cap, int32_t* frame,
                                                                 uint32_t* strength, int32_t* count) {
    __shared__ uint32_t sh[PEAK_TILE + 2 * PEAK_HALO];
    __shared__ int wave_count[PEAK_THREADS / 64];
    const int64_t t = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t nf = n_frames[t];
    if (nf < 0 || nf > D_ld) {                                   // (uniform) a video that does not fit: no list
        if (tid == 0) count[t] = -1;
        return;
    }
    const uint32_t* e = D + t * D_ld;
    const uint32_t th = thr[t];
    int64_t n_out = 0;                                           // (uniform)
    for (int64_t f0 = 0; f0 < nf; f0 += PEAK_TILE) {
        __syncthreads();                                         // the pass before has read sh
        for (int i = tid; i < PEAK_TILE + 2 * PEAK_HALO; i += PEAK_THREADS) {
            const int64_t g = f0 - PEAK_HALO + i;
            sh[i] = (g >= 0 && g < nf) ? e[g] : 0u;
        }
        __syncthreads();
        for (int j = 0; j < PEAK_TILE / PEAK_THREADS; ++j) {
            const int64_t f = f0 + j * PEAK_THREADS + tid;
            bool peak = false;
            uint32_t x = 0u;
            if (f < nf) {
                const int c = PEAK_HALO + j * PEAK_THREADS + tid;                    // sh[c] = D[f]
                x = sh[c];
                peak = x > 0u && x >= th;
                const int lo = (int)(f - w_max < 0 ? f : w_max), hi = (int)(f + w_max >= nf ? nf - 1 - f : w_max);
                for (int d = 1; d <= lo; ++d) peak = peak && x > sh[c - d];
                for (int d = 1; d <= hi; ++d) peak = peak && x >= sh[c + d];
                if (peak) {                                      // few frames get here: at most one in w_max + 1
                    const int64_t a = f - w_avg < 1 ? 1 : f - w_avg, b = f + w_avg >= nf ? nf - 1 : f + w_avg;     // [a, b] inside [1, nf)
                    int64_t s = 0, n = 0;
                    for (int64_t g = a; g <= b; ++g)
                        if (g != f) { s += (int64_t)sh[c + (int)(g - f)]; ++n; }
                    peak = n == 0 || 256ll * (int64_t)x * n >= (int64_t)ratio_q8 * s;
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
            if (peak && at < cap) {
                frame[t * cap + at] = (int32_t)f;
                strength[t * cap + at] = x;
            }
            n_out += total;
            __syncthreads();                                     // wave_count is rewritten by the next j
        }
    }
    if (tid == 0) count[t] = (int32_t)(n_out < cap ? n_out : cap);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int made_frame_hist(const uint8_t* frames, int64_t frames_len, const MadeCutFrameDesc* desc, int64_t n_frames, uint32_t* hist,
                               void* stream) {
    MADE_REQUIRE(n_frames >= 0, "made_frame_hist: n_frames is negative");
    MADE_REQUIRE(frames_len >= 0, "made_frame_hist: frames_len is negative");
    if (n_frames == 0) return MADE_OK;
    MADE_REQUIRE(frames && desc && hist, "made_frame_hist: null pointer (frames, desc or hist)");
    MADE_REQUIRE(n_frames < (1LL << 21), "made_frame_hist: n_frames must be below 2^21, got %lld", (long long)n_frames);
    MADE_REQUIRE(frames_len >= 3, "made_frame_hist: frames_len = %lld holds no frame (a pixel is 3 bytes)", (long long)frames_len);
    // the workgroups a frame gets: enough for a frame of the mean size to give every one a single chunk; a larger frame's take more
    // (the descriptors are on the device: the host sees the byte count alone)
    int64_t per_frame = (frames_len / (3 * n_frames) + CHUNK_PIXELS - 1) / CHUNK_PIXELS;
    per_frame = per_frame < 1 ? 1 : per_frame > MAX_PIXELS / CHUNK_PIXELS ? MAX_PIXELS / CHUNK_PIXELS : per_frame;
    MADE_REQUIRE(n_frames * per_frame < (1LL << 31), "made_frame_hist: n_frames * workgroups per frame must be below 2^31");
    const int st = made_memset_async(hist, 0, n_frames * HIST_BINS * (int64_t)sizeof(uint32_t), stream);
    if (st != MADE_OK) return st;
    const char* merge = made_variant_env("MADE_CUTS_MERGE");   // "0": an LDS add per pixel, no run merging (docs/EXPERIMENTS.md)
    auto kernel = merge && merge[0] == '0' ? frame_hist_kernel<false> : frame_hist_kernel<true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n_frames * per_frame)), dim3(HIST_THREADS), 0, (hipStream_t)stream, frames, frames_len, desc,
                       (int)per_frame, hist);
    return made_check_launch("made_frame_hist");
}

extern "C" int made_hist_distance(const uint32_t* hist, const uint8_t* first_of_video, int64_t n_frames, uint32_t* D, void* stream) {
    MADE_REQUIRE(n_frames >= 0, "made_hist_distance: n_frames is negative");
    if (n_frames == 0) return MADE_OK;
    MADE_REQUIRE(hist && first_of_video && D, "made_hist_distance: null pointer (hist, first_of_video or D)");
    MADE_REQUIRE(aligned16(hist), "made_hist_distance: hist must be 16-byte aligned");
    MADE_REQUIRE(n_frames < (1LL << 31), "made_hist_distance: n_frames must be below 2^31, got %lld", (long long)n_frames);
    hipLaunchKernelGGL(hist_distance_kernel, dim3((unsigned)((n_frames + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint4*)hist,
                       first_of_video, n_frames, D);
    return made_check_launch("made_hist_distance");
}

extern "C" int made_cut_peaks(const uint32_t* D, int64_t D_ld, const int32_t* n_frames, int64_t N, const uint32_t* thr, int32_t w_max,
                              int32_t w_avg, int32_t ratio_q8, int64_t cap, int32_t* frame, uint32_t* strength, int32_t* count, void* stream) {
    MADE_REQUIRE(N >= 0 && D_ld >= 0 && cap >= 0, "made_cut_peaks: negative size (N, D_ld or cap)");
    MADE_REQUIRE(w_max >= 1 && w_max <= 64, "made_cut_peaks: w_max must lie in [1, 64], got %d", (int)w_max);
    MADE_REQUIRE(w_avg >= 1 && w_avg <= PEAK_HALO, "made_cut_peaks: w_avg must lie in [1, %d], got %d", PEAK_HALO, (int)w_avg);
    MADE_REQUIRE(ratio_q8 >= 0 && ratio_q8 <= 65535, "made_cut_peaks: ratio_q8 must lie in [0, 65535], got %d", (int)ratio_q8);
    if (N == 0) return MADE_OK;
    MADE_REQUIRE(n_frames && thr && count && (D || D_ld == 0) && ((frame && strength) || cap == 0),
                 "made_cut_peaks: null pointer (D, n_frames, thr, frame, strength or count)");
    MADE_REQUIRE(cap >= (D_ld + w_max) / (w_max + 1), "made_cut_peaks: cap must be >= ceil(D_ld / (w_max + 1)) = %lld, got %lld",
                 (long long)((D_ld + w_max) / (w_max + 1)), (long long)cap);
    MADE_REQUIRE(N < (1LL << 31) && D_ld < (1LL << 31), "made_cut_peaks: N and D_ld must be below 2^31");
    hipLaunchKernelGGL(cut_peaks_kernel, dim3((unsigned)N), dim3(PEAK_THREADS), 0, (hipStream_t)stream, D, D_ld, n_frames, thr, (int)w_max,
                       (int)w_avg, (int)ratio_q8, cap, frame, strength, count);
    return made_check_launch("made_cut_peaks");
}
