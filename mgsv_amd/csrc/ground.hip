// Grounding: the best K tracks of every video row of the similarity matrix (made_topk_groups; made_topk_groups_masked under the
// per-video eligibility bits of made_eligibility) and the localization batch of arbitrary (video, track) pairs assembled from
// per-item tower outputs (made_gather_pairs).  Neither has a counterpart in the
// reference, which predicts a moment only in the ground-truth track.
#include "common.h"

namespace {

constexpr int GT = 256;                 // threads per workgroup; the final sort gives every thread one candidate (K <= 256)
constexpr int CAP = 32768;              // items one workgroup selects from: 128 KiB of keys in LDS
constexpr uint32_t SLOT_OUT = 0xFFFFFFFFu;
constexpr uint32_t TIE = 0x40000000u;   // group table: TIE + (lowest column of the group at the threshold score)
constexpr uint32_t TIE_NONE = 0x7FFFFFFFu;

struct TopkShared {
    int hist[256];
    uint32_t cand_key[256];
    int cand_col[256];
    int wsum[GT / 64];
    int sel[2];
    int cnt;
};

// Histogram add with the lanes of a wave that share a bin folded into one atomic (the top bytes of similarity scores sit in
// one or two bins, where plain LDS atomics serialise 64-fold); after a few distinct bins the rest fall back to plain atomics.
__device__ __forceinline__ void hist_add(int* hist, bool active, int bin) {
    const int lane = threadIdx.x & 63;
    for (int it = 0; it < 4; ++it) {
        const unsigned long long act = __ballot(active);
        if (act == 0ull) return;
        const int leader = __ffsll((long long)act) - 1;
        const int b0 = __shfl(bin, leader);
        const unsigned long long same = __ballot(active && bin == b0);
        if (lane == leader) atomicAdd(&hist[b0], __popcll(same));
        if (bin == b0) active = false;
    }
    if (active) atomicAdd(&hist[bin], 1);
}

// The kk-th largest key of v[0..n) (1 <= kk <= n), MSB-first radix select over 8-bit digits.  Returns the key t and writes to
// *need how many items equal to t belong to the top kk.
__device__ uint32_t radix_select(const uint32_t* v, int n, int kk, TopkShared& sh, int* need_out) {
    uint32_t prefix = 0u, mask = 0u;
    int need = kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = threadIdx.x; b < 256; b += GT) sh.hist[b] = 0;
        __syncthreads();
        for (int base = 0; base < n; base += GT) {
            const int i = base + threadIdx.x;
            const uint32_t x = i < n ? v[i] : 0u;
            hist_add(sh.hist, i < n && (x & mask) == prefix, (int)((x >> shift) & 255u));
        }
        __syncthreads();
        if (threadIdx.x < 64) {                              // lane l owns bins 255-4l .. 252-4l (descending)
            const int lane = threadIdx.x;
            int c[4], s = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { c[q] = sh.hist[255 - 4 * lane - q]; s += c[q]; }
            int incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            const int excl = incl - s;
            if (excl < need && incl >= need) {
                int cum = excl;
                for (int q = 0; q < 4; ++q) {
                    if (cum + c[q] >= need) { sh.sel[0] = 255 - 4 * lane - q; sh.sel[1] = need - cum; break; }
                    cum += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= (uint32_t)sh.sel[0] << shift;
        mask |= 0xFFu << shift;
        need = sh.sel[1];
        __syncthreads();
    }
    *need_out = need;
    return prefix;
}

// Exclusive prefix count of `flag` over the workgroup (thread order); *total = the workgroup's count.
__device__ __forceinline__ int block_excl_count(bool flag, TopkShared& sh, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) sh.wsum[w] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < GT / 64; ++q) { off += q < w ? sh.wsum[q] : 0; tot += sh.wsum[q]; }
    __syncthreads();
    *total = tot;
    return off + pre;
}

// Key of column j of a row under an eligibility mask (made_eligibility's layout: bit j & 31 of word j >> 5): 0, "no item", when the
// bit is clear.  Every read of a score in the masked instantiations goes through here; the unmasked ones read the score alone.
template <bool MASKED>
__device__ __forceinline__ uint32_t column_key(const float* s, const uint32_t* bits, int j) {
    if constexpr (MASKED) {
        if (!((bits[j >> 5] >> (j & 31)) & 1u)) return 0u;
    }
    return score_key(s[j]);
}

// One workgroup selects the best K of one row's items and writes them sorted (score descending, column ascending).
//   mode 0: columns [c0, c0 + n) of the row, one item each;
//   mode 1: groups -- item g = group g, key = the group's best column, column = the lowest column attaining it;
//   mode 2: the sorted candidate lists of a previous pass (key, column), item order ascending in column among equal keys.
// Workgroup x: row = x / nblk, block b = x % nblk.  final_out: idx / score [row, K]; else key / column candidates [row, nblk, K].
// MASKED: columns whose bit of mask [row, mask_ld words] is clear are no items (modes 0 and 1; mode 2 sees candidate lists only).
template <bool MASKED>
__global__ __launch_bounds__(GT) void topk_kernel(const float* sims, int64_t ld, const uint32_t* mask, int64_t mask_ld,
                                                  const int32_t* gid, int Nm, int G,
                                                  const uint32_t* ckey_in, const int32_t* ccol_in, int n_in, int per_block,
                                                  int K, int mode, int nblk, int32_t* idx_out, float* score_out,
                                                  uint32_t* ckey_out, int32_t* ccol_out) {
    extern __shared__ uint32_t v[];
    __shared__ TopkShared sh;
    const int64_t row = blockIdx.x / nblk;
    const int b = blockIdx.x % nblk;
    const float* s = sims ? sims + row * ld : nullptr;
    const uint32_t* mb = MASKED ? mask + row * mask_ld : nullptr;
    int n, i0 = 0;
    if (mode == 0) {
        i0 = b * per_block;
        n = min(per_block, Nm - i0);
        for (int i = threadIdx.x; i < n; i += GT) v[i] = column_key<MASKED>(s, mb, i0 + i);
    } else if (mode == 1) {
        n = G;
        for (int g = threadIdx.x; g < G; g += GT) v[g] = 0u;
        __syncthreads();
        for (int j = threadIdx.x; j < Nm; j += GT) {
            const int g = gid[j];
            if ((unsigned)g < (unsigned)G) atomicMax(&v[g], column_key<MASKED>(s, mb, j));
        }
    } else {
        i0 = b * per_block;
        n = min(per_block, n_in - i0);
        const uint32_t* kin = ckey_in + row * n_in + i0;
        for (int i = threadIdx.x; i < n; i += GT) v[i] = kin[i];
    }
    if (threadIdx.x == 0) sh.cnt = 0;
    __syncthreads();
    const int kk = min(K, n);
    int m = 0;
    const uint32_t t = radix_select(v, n, kk, sh, &m);
    const int32_t* cin = mode == 2 ? ccol_in + row * n_in + i0 : nullptr;

    // items above the threshold (fewer than kk of them), then the m lowest columns among the items AT the threshold
    if (mode == 1) {
        for (int g = threadIdx.x; g < G; g += GT) {
            const uint32_t k = v[g];
            if (k > t) {
                const int slot = atomicAdd(&sh.cnt, 1);
                sh.cand_key[slot] = k; sh.cand_col[slot] = 0x7FFFFFFF; v[g] = (uint32_t)slot;
            } else {
                v[g] = (k == t && t != 0u) ? TIE_NONE : SLOT_OUT;
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < Nm; j += GT) {           // representative columns: lowest index attaining the group's maximum
            const int g = gid[j];
            if ((unsigned)g >= (unsigned)G) continue;
            const uint32_t e = v[g];
            if (e == SLOT_OUT) continue;
            const uint32_t k = column_key<MASKED>(s, mb, j);
            if (e < 256u) { if (k == sh.cand_key[e]) atomicMin(&sh.cand_col[e], j); }
            else if (k == t) atomicMin(&v[g], TIE + (uint32_t)j);
        }
    } else {
        for (int i = threadIdx.x; i < n; i += GT) {
            const uint32_t k = v[i];
            if (k > t) {
                const int slot = atomicAdd(&sh.cnt, 1);
                sh.cand_key[slot] = k; sh.cand_col[slot] = mode == 0 ? i0 + i : cin[i];
            }
        }
    }
    __syncthreads();
    const int n_above = sh.cnt;
    int taken = 0;
    const int want = t != 0u ? kk - n_above : 0;
    const int scan_n = mode == 1 ? Nm : n;
    for (int base = 0; base < scan_n && taken < want; base += GT) {     // (uniform: `taken` is the same in every thread)
        const int i = base + threadIdx.x;
        bool f = false;
        if (i < scan_n) {
            if (mode == 1) { const int g = gid[i]; f = (unsigned)g < (unsigned)G && v[g] == TIE + (uint32_t)i; }
            else f = v[i] == t;
        }
        int tot;
        const int pos = block_excl_count(f, sh, &tot);
        if (f && taken + pos < want) {
            sh.cand_key[n_above + taken + pos] = t;
            sh.cand_col[n_above + taken + pos] = mode == 2 ? cin[i] : (mode == 0 ? i0 + i : i);
        }
        taken += tot;
    }
    __syncthreads();
    const int total = n_above + min(taken, want);

    // rank sort of the (at most 256) candidates; the tail past `total` is filled
    const int64_t o = (row * nblk + b) * (int64_t)K;
    if ((int)threadIdx.x < total) {
        const uint32_t k = sh.cand_key[threadIdx.x];
        const int c = sh.cand_col[threadIdx.x];
        int r = 0;
        for (int q = 0; q < total; ++q) {
            const uint32_t kq = sh.cand_key[q];
            r += (kq > k || (kq == k && sh.cand_col[q] < c)) ? 1 : 0;
        }
        if (idx_out) { idx_out[o + r] = c; score_out[o + r] = key_score(k); }
        else { ckey_out[o + r] = k; ccol_out[o + r] = c; }
    }
    for (int r = total + threadIdx.x; r < K; r += GT) {
        if (idx_out) { idx_out[o + r] = -1; score_out[o + r] = -INFINITY; }
        else { ckey_out[o + r] = 0u; ccol_out[o + r] = -1; }
    }
}

}  // namespace

namespace {

// One workgroup per pair: frame tokens, segment tokens (16-byte accesses), the two masks and the two clip vectors.  A pair with
// an index outside [0, Nv) x [0, Nm) is written as all padding (zeros) and nothing of the inputs is read for it.
__global__ __launch_bounds__(256) void gather_pairs_kernel(const int32_t* vi, const int32_t* mi, int64_t Nv, int64_t Nm,
                                                           const uint4* v_tok, int64_t v_tok_s, const float* v_mask, int64_t v_mask_s,
                                                           const float* v_vec, int64_t v_vec_s,
                                                           const uint4* m_tok, int64_t m_tok_s, const float* m_mask, int64_t m_mask_s,
                                                           const float* m_vec, int64_t m_vec_s, int Tv, int Ta, int D, int64_t nv16,
                                                           int64_t na16, uint4* frame_out, int64_t frame_s, uint4* seg_out, int64_t seg_s,
                                                           float* fmask_out, float* smask_out, float* video_out, float* music_out) {
    const int64_t p = blockIdx.x;
    const int64_t a = vi[p], c = mi[p];
    const bool ok = a >= 0 && a < Nv && c >= 0 && c < Nm;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    const uint4* vt = v_tok + (ok ? a * v_tok_s : 0);
    const uint4* mt = m_tok + (ok ? c * m_tok_s : 0);
    uint4* fo = frame_out + p * frame_s;
    uint4* so = seg_out + p * seg_s;
    for (int64_t i = threadIdx.x; i < nv16; i += 256) fo[i] = ok ? vt[i] : z;
    for (int64_t i = threadIdx.x; i < na16; i += 256) so[i] = ok ? mt[i] : z;
    for (int i = threadIdx.x; i < Tv; i += 256) fmask_out[p * Tv + i] = ok ? v_mask[a * v_mask_s + i] : 0.f;
    for (int i = threadIdx.x; i < Ta; i += 256) smask_out[p * Ta + i] = ok ? m_mask[c * m_mask_s + i] : 0.f;
    for (int i = threadIdx.x; i < D; i += 256) {
        video_out[p * D + i] = ok ? v_vec[a * v_vec_s + i] : 0.f;
        music_out[p * D + i] = ok ? m_vec[c * m_vec_s + i] : 0.f;
    }
}

constexpr int MERGE_K = 256;            // entries of one list at most (made_topk_groups' K limit)

struct MergeListShared {
    uint64_t key[2 * MERGE_K];          // (score key, 0x7FFFFFFF - column) of an entry's best column; 0 = an empty entry
    int src[MERGE_K];                   // output slot -> entry (a: 0 .. Ka-1, b: Ka .. Ka+Kb-1)
};

// One workgroup per row merges two sorted lists of entries (made_topk_merge).  Rank by counting over the Ka + Kb <= 512 keys in
// LDS (every thread reads the same key: a broadcast), then the payload of the first K entries is copied slot by slot, so the
// stores of a row are contiguous.  Equal keys (empty entries; lists that break the disjoint-columns contract) rank in entry
// order: the ranks are a permutation of 0 .. Ka+Kb-1 whatever the input, and every output slot is written exactly once.
template <int V>                        // V = 4: 16-byte accesses (w % 4 == 0, every buffer 16-byte aligned); V = 1: 4-byte
__global__ __launch_bounds__(GT) void topk_merge_kernel(const int32_t* a_col, const float* a_score, int Ka, const int32_t* b_col,
                                                        const float* b_score, int Kb, int32_t col_offset, int w, int K,
                                                        int32_t* out_col, float* out_score) {
    __shared__ MergeListShared sh;
    const int64_t row = blockIdx.x;
    const int n = Ka + Kb;
    const int32_t* ac = a_col + row * Ka * w;
    const float* as = a_score + row * Ka * w;
    const int32_t* bc = b_col + row * Kb * w;
    const float* bs = b_score + row * Kb * w;
    for (int i = threadIdx.x; i < n; i += GT) {
        const bool isb = i >= Ka;
        const int64_t e = (int64_t)(isb ? i - Ka : i) * w;
        const int c = isb ? bc[e] : ac[e];
        uint64_t k = 0ull;
        if (c >= 0) {
            const float s = isb ? bs[e] : as[e];
            const uint32_t col = (uint32_t)c + (isb ? (uint32_t)col_offset : 0u);
            k = ((uint64_t)score_key(s) << 32) | (uint32_t)(0x7FFFFFFFu - col);
        }
        sh.key[i] = k;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += GT) {
        const uint64_t k = sh.key[i];
        int r = 0;
        for (int q = 0; q < n; ++q) {
            const uint64_t kq = sh.key[q];
            r += (kq > k || (kq == k && q < i)) ? 1 : 0;
        }
        if (r < K) sh.src[r] = i;
    }
    __syncthreads();
    const int filled = min(n, K);
    const int wv = w / V;                                        // payload vectors per entry
    const int64_t o = row * K * w;
    for (int x = threadIdx.x; x < K * wv; x += GT) {
        const int r = x / wv, j = (x - r * wv) * V;
        int32_t c[V];
        float s[V];
#pragma unroll
        for (int t = 0; t < V; ++t) { c[t] = -1; s[t] = -INFINITY; }
        const int i = r < filled ? sh.src[r] : -1;
        if (i >= 0 && sh.key[i] != 0ull) {
            const bool isb = i >= Ka;
            const int64_t e = (int64_t)(isb ? i - Ka : i) * w + j;
            const int32_t* pc = isb ? bc + e : ac + e;
            const float* ps = isb ? bs + e : as + e;
            if constexpr (V == 4) {
                const int4 cv = *(const int4*)pc;
                const float4 sv = *(const float4*)ps;
                c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
                s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
            } else {
                c[0] = *pc; s[0] = *ps;
            }
            if (isb) {
#pragma unroll
                for (int t = 0; t < V; ++t) c[t] = c[t] >= 0 ? (int32_t)((uint32_t)c[t] + (uint32_t)col_offset) : c[t];
            }
        }
        if constexpr (V == 4) {
            *(int4*)(out_col + o + (int64_t)r * w + j) = make_int4(c[0], c[1], c[2], c[3]);
            *(float4*)(out_score + o + (int64_t)r * w + j) = make_float4(s[0], s[1], s[2], s[3]);
        } else {
            out_col[o + (int64_t)r * w + j] = c[0];
            out_score[o + (int64_t)r * w + j] = s[0];
        }
    }
}

int64_t topk_blocks(int64_t Nm) { return (Nm + CAP - 1) / CAP; }

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

bool overlaps(const void* p, int64_t pn, const void* q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

}  // namespace

extern "C" int64_t made_topk_groups_ws_bytes(int64_t Nv, int64_t Nm, int64_t K) {
    if (Nv <= 0 || Nm <= CAP || K < 1 || K > 256) return 0;
    const int64_t nb0 = topk_blocks(Nm);
    const int64_t fan = (CAP / K) * K;
    const int64_t nb1 = (nb0 * K + fan - 1) / fan;
    return (nb0 + nb1) * Nv * K * 8;
}

namespace {

// made_topk_groups and made_topk_groups_masked: the same launches, of the unmasked or the masked instantiation
template <bool MASKED>
int topk_groups_launch(const float* sims, int64_t ld, const int32_t* group_id, const uint32_t* bits, int64_t bits_ld, int64_t Nv,
                       int64_t Nm, int64_t n_groups, int64_t K, int32_t* idx_out, float* score_out, void* ws, int64_t ws_bytes,
                       void* stream) {
    MADE_REQUIRE(sims && idx_out && score_out, "made_topk_groups: null pointer");
    MADE_REQUIRE(Nv >= 0 && Nm > 0 && ld >= Nm, "made_topk_groups: bad dims (Nv >= 0, Nm > 0, ld >= Nm)");
    MADE_REQUIRE(K >= 1 && K <= 256, "made_topk_groups: K must lie in [1, 256]");
    MADE_REQUIRE(Nm <= (1LL << 24), "made_topk_groups: at most 2^24 columns");
    if (group_id) MADE_REQUIRE(n_groups >= 1 && n_groups <= 32768, "made_topk_groups: n_groups must lie in [1, 32768] (LDS table)");
    const int64_t need = group_id ? 0 : made_topk_groups_ws_bytes(Nv, Nm, K);
    MADE_REQUIRE(need == 0 || (ws && ws_bytes >= need), "made_topk_groups: workspace of %lld bytes needed", (long long)need);
    MADE_REQUIRE(Nv * topk_blocks(Nm) < (1LL << 31), "made_topk_groups: too many rows");
    if (MASKED) MADE_REQUIRE(bits_ld >= (Nm + 31) / 32, "made_topk_groups_masked: bits_ld must be >= ceil(Nm / 32) words");
    if (Nv == 0) return MADE_OK;
    static bool attr_done = false;                               // (one per instantiation; the later passes are unmasked)
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void*)topk_kernel<MASKED>, hipFuncAttributeMaxDynamicSharedMemorySize, CAP * 4);
        if (MASKED) (void)hipFuncSetAttribute((const void*)topk_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, CAP * 4);
        attr_done = true;
    }
    const hipStream_t st = (hipStream_t)stream;
    if (group_id) {
        hipLaunchKernelGGL(topk_kernel<MASKED>, dim3((unsigned)Nv), dim3(GT), (size_t)n_groups * 4, st, sims, ld, bits, bits_ld, group_id, (int)Nm, (int)n_groups,
                           (const uint32_t*)nullptr, (const int32_t*)nullptr, 0, 0, (int)K, 1, 1, idx_out, score_out, (uint32_t*)nullptr,
                           (int32_t*)nullptr);
        return made_check_launch("made_topk_groups");
    }
    if (Nm <= CAP) {
        hipLaunchKernelGGL(topk_kernel<MASKED>, dim3((unsigned)Nv), dim3(GT), (size_t)Nm * 4, st, sims, ld, bits, bits_ld, (const int32_t*)nullptr, (int)Nm, 0,
                           (const uint32_t*)nullptr, (const int32_t*)nullptr, 0, (int)Nm, (int)K, 0, 1, idx_out, score_out,
                           (uint32_t*)nullptr, (int32_t*)nullptr);
        return made_check_launch("made_topk_groups");
    }
    // long rows: the best K of every block of CAP columns, then passes over the blocks' sorted candidate lists (CAP / K lists per
    // workgroup) until one list per row is left.  Workspace: lists of pass 0 (nb0 per row) | lists of pass 1 (nb1 per row); later
    // passes alternate between the two (each has fewer lists than the one before).
    const int64_t nb0 = topk_blocks(Nm);
    const int64_t fan = (CAP / K) * K;
    const int64_t nb1 = (nb0 * K + fan - 1) / fan;
    char* base = (char*)ws;
    uint32_t* keys[2] = {(uint32_t*)base, (uint32_t*)(base + nb0 * Nv * K * 8)};
    int32_t* cols[2] = {(int32_t*)(base + nb0 * Nv * K * 4), (int32_t*)(base + nb0 * Nv * K * 8 + nb1 * Nv * K * 4)};
    hipLaunchKernelGGL(topk_kernel<MASKED>, dim3((unsigned)(Nv * nb0)), dim3(GT), (size_t)CAP * 4, st, sims, ld, bits, bits_ld, (const int32_t*)nullptr, (int)Nm, 0,
                       (const uint32_t*)nullptr, (const int32_t*)nullptr, 0, CAP, (int)K, 0, (int)nb0, (int32_t*)nullptr, (float*)nullptr,
                       keys[0], cols[0]);
    int64_t nb = nb0;
    int cur = 0;
    while (true) {
        const int64_t n_in = nb * K;
        const int64_t nxt = (n_in + fan - 1) / fan;
        const bool last = nxt == 1;
        hipLaunchKernelGGL(topk_kernel<false>, dim3((unsigned)(Nv * nxt)), dim3(GT), (size_t)min(n_in, fan) * 4, st, (const float*)nullptr, ld,
                           (const uint32_t*)nullptr, (int64_t)0, (const int32_t*)nullptr, (int)Nm, 0, (const uint32_t*)keys[cur], (const int32_t*)cols[cur], (int)n_in, (int)fan,
                           (int)K, 2, (int)nxt, last ? idx_out : (int32_t*)nullptr, last ? score_out : (float*)nullptr,
                           last ? (uint32_t*)nullptr : keys[cur ^ 1], last ? (int32_t*)nullptr : cols[cur ^ 1]);
        if (last) break;
        nb = nxt;
        cur ^= 1;
    }
    return made_check_launch("made_topk_groups");
}

}  // namespace

extern "C" int made_topk_groups(const float* sims, int64_t ld, const int32_t* group_id, int64_t Nv, int64_t Nm, int64_t n_groups,
                                int64_t K, int32_t* idx_out, float* score_out, void* ws, int64_t ws_bytes, void* stream) {
    return topk_groups_launch<false>(sims, ld, group_id, nullptr, 0, Nv, Nm, n_groups, K, idx_out, score_out, ws, ws_bytes, stream);
}

extern "C" int made_topk_groups_masked(const float* sims, int64_t ld, const int32_t* group_id, const uint32_t* bits, int64_t bits_ld,
                                       int64_t Nv, int64_t Nm, int64_t n_groups, int64_t K, int32_t* idx_out, float* score_out,
                                       void* ws, int64_t ws_bytes, void* stream) {
    if (!bits) return topk_groups_launch<false>(sims, ld, group_id, nullptr, 0, Nv, Nm, n_groups, K, idx_out, score_out, ws, ws_bytes, stream);
    return topk_groups_launch<true>(sims, ld, group_id, bits, bits_ld, Nv, Nm, n_groups, K, idx_out, score_out, ws, ws_bytes, stream);
}

namespace {

constexpr int ET = 256;                 // columns of one workgroup of made_eligibility: one per thread, 2 words of 32 per wave
constexpr int E_BLOCKS = 2048;          // workgroups aimed at: the rows are dealt over as many as the column tiles leave room for

// Workgroup (x, y): columns [256 x, 256 x + 256), rows y, y + gridDim.y, ...  A thread keeps its column's attributes in registers
// for every row; a row's constraints are uniform loads.  A wave's 64 tests of a row are one ballot = two words of bits_out; the
// OR over the workgroup's rows stays in registers and costs one atomicOr per word at the end.
__global__ __launch_bounds__(ET) void eligibility_kernel(const int64_t* col_tags, const float* col_length, const int32_t* col_key,
                                                         const int64_t* row_all, const int64_t* row_any, const int64_t* row_forbid,
                                                         const float* row_min, const float* row_max, const int32_t* ex_start,
                                                         const int32_t* ex_keys, int n_ex, int Nv, int Nm, uint32_t* bits_out,
                                                         int64_t ld_words, uint32_t* col_any_out) {
    const int c = blockIdx.x * ET + threadIdx.x;
    const bool there = c < Nm;
    const int lane = threadIdx.x & 63;
    const uint64_t tags = there && col_tags ? (uint64_t)col_tags[c] : 0ull;
    const float len = there && col_length ? col_length[c] : 0.f;
    const int key = there && col_key ? col_key[c] : 0;
    const int word = (blockIdx.x * ET + (threadIdx.x & ~63)) / 32 + (lane >> 5);      // the word lanes 0 and 32 of this wave write
    const bool writer = (lane & 31) == 0 && word < (Nm + 31) / 32;
    unsigned long long any = 0ull;
    for (int i = blockIdx.y; i < Nv; i += gridDim.y) {
        bool ok = there;
        if (col_tags) {
            const uint64_t all = row_all ? (uint64_t)row_all[i] : 0ull;
            const uint64_t some = row_any ? (uint64_t)row_any[i] : 0ull;
            const uint64_t none = row_forbid ? (uint64_t)row_forbid[i] : 0ull;
            ok = ok && (tags & all) == all && (some == 0ull || (tags & some) != 0ull) && (tags & none) == 0ull;
        }
        if (row_min) ok = ok && len >= row_min[i];               // (a NaN length fails a bound that is tested)
        if (row_max) ok = ok && len <= row_max[i];
        if (ex_start) {
            int a = min(max(ex_start[i], 0), n_ex);              // uniform: an empty list costs nothing more
            const int end = min(max(ex_start[i + 1], a), n_ex);
            if (a < end && ok) {
                int b = end;
                while (a < b) {                                  // first position whose key is >= key
                    const int m = a + ((b - a) >> 1);
                    if (ex_keys[m] < key) a = m + 1; else b = m;
                }
                ok = !(a < end && ex_keys[a] == key);
            }
        }
        const unsigned long long bal = __ballot(ok);
        any |= bal;
        if (bits_out && writer) bits_out[(int64_t)i * ld_words + word] = (uint32_t)(bal >> (lane & 32));
    }
    if (col_any_out && writer) {
        const uint32_t wd = (uint32_t)(any >> (lane & 32));
        if (wd) atomicOr(&col_any_out[word], wd);
    }
}

}  // namespace

extern "C" int made_eligibility(const int64_t* col_tags, const float* col_length, const int32_t* col_key, const int64_t* row_all,
                                const int64_t* row_any, const int64_t* row_forbid, const float* row_min, const float* row_max,
                                const int32_t* ex_start, const int32_t* ex_keys, int64_t n_ex_keys, int64_t Nv, int64_t Nm,
                                uint32_t* bits_out, int64_t ld_words, uint32_t* col_any_out, void* stream) {
    MADE_REQUIRE(Nv >= 0 && Nm > 0 && Nv < (1LL << 31) && Nm < (1LL << 31) - 256, "made_eligibility: bad dims (0 <= Nv < 2^31, 0 < Nm < 2^31 - 256)");
    MADE_REQUIRE(bits_out || col_any_out, "made_eligibility: no output (bits_out and col_any_out are both null)");
    MADE_REQUIRE(!bits_out || ld_words >= (Nm + 31) / 32, "made_eligibility: ld_words must be >= ceil(Nm / 32)");
    MADE_REQUIRE(col_length || (!row_min && !row_max), "made_eligibility: a length bound (row_min / row_max) needs col_length");
    MADE_REQUIRE(col_key || !ex_start, "made_eligibility: exclusion lists (ex_start) need col_key");
    MADE_REQUIRE(col_tags || (!row_all && !row_any && !row_forbid), "made_eligibility: a tag pattern (row_all / row_any / row_forbid) needs col_tags");
    MADE_REQUIRE(!ex_start || (n_ex_keys >= 0 && n_ex_keys < (1LL << 31) && (ex_keys || n_ex_keys == 0)),
                 "made_eligibility: ex_start needs ex_keys [n_ex_keys], 0 <= n_ex_keys < 2^31");
    if (Nv == 0) return MADE_OK;
    const int64_t tiles = (Nm + ET - 1) / ET;
    const int64_t ny = max((int64_t)1, min(min(Nv, (int64_t)65535), E_BLOCKS / tiles));
    hipLaunchKernelGGL(eligibility_kernel, dim3((unsigned)tiles, (unsigned)ny), dim3(ET), 0, (hipStream_t)stream, col_tags, col_length,
                       col_key, row_all, row_any, row_forbid, row_min, row_max, ex_start, ex_keys, (int)(ex_start ? n_ex_keys : 0), (int)Nv,
                       (int)Nm, bits_out, ld_words, col_any_out);
    return made_check_launch("made_eligibility");
}

extern "C" int made_topk_merge(const int32_t* a_col, const float* a_score, int64_t Ka, const int32_t* b_col, const float* b_score,
                               int64_t Kb, int64_t col_offset, int64_t Nv, int64_t w, int64_t K, int32_t* out_col, float* out_score,
                               void* stream) {
    MADE_REQUIRE(out_col && out_score, "made_topk_merge: null output pointer");
    MADE_REQUIRE(K >= 1 && K <= MERGE_K, "made_topk_merge: K must lie in [1, 256]");
    MADE_REQUIRE(Ka >= 0 && Ka <= MERGE_K && Kb >= 0 && Kb <= MERGE_K, "made_topk_merge: Ka and Kb must lie in [0, 256]");
    MADE_REQUIRE(w >= 1 && w <= 16, "made_topk_merge: w must lie in [1, 16]");
    MADE_REQUIRE(Nv >= 0 && Nv < (1LL << 31), "made_topk_merge: bad dims (0 <= Nv < 2^31)");
    MADE_REQUIRE(col_offset >= 0 && col_offset < (1LL << 31), "made_topk_merge: col_offset must lie in [0, 2^31)");
    MADE_REQUIRE((Ka == 0 || (a_col && a_score)) && (Kb == 0 || (b_col && b_score)), "made_topk_merge: null pointer (a list that is not empty)");
    const int64_t na = Nv * Ka * w * 4, nb = Nv * Kb * w * 4, no = Nv * K * w * 4;
    MADE_REQUIRE((const void*)out_col != (const void*)out_score && !overlaps(out_col, no, out_score, no) &&
                 !overlaps(out_col, no, a_col, na) && !overlaps(out_col, no, a_score, na) && !overlaps(out_col, no, b_col, nb) &&
                 !overlaps(out_col, no, b_score, nb) && !overlaps(out_score, no, a_col, na) && !overlaps(out_score, no, a_score, na) &&
                 !overlaps(out_score, no, b_col, nb) && !overlaps(out_score, no, b_score, nb),
                 "made_topk_merge: the outputs must not alias the inputs or each other");
    if (Nv == 0) return MADE_OK;
    const bool v4 = w % 4 == 0 && aligned16(a_col) && aligned16(a_score) && aligned16(b_col) && aligned16(b_score) &&
                    aligned16(out_col) && aligned16(out_score);
    const hipStream_t st = (hipStream_t)stream;
    if (v4)
        hipLaunchKernelGGL(topk_merge_kernel<4>, dim3((unsigned)Nv), dim3(GT), 0, st, a_col, a_score, (int)Ka, b_col, b_score, (int)Kb,
                           (int32_t)col_offset, (int)w, (int)K, out_col, out_score);
    else
        hipLaunchKernelGGL(topk_merge_kernel<1>, dim3((unsigned)Nv), dim3(GT), 0, st, a_col, a_score, (int)Ka, b_col, b_score, (int)Kb,
                           (int32_t)col_offset, (int)w, (int)K, out_col, out_score);
    return made_check_launch("made_topk_merge");
}

namespace {

struct CandShared {
    uint64_t key[GT];                   // (score key, 0x7FFFFFFF - column) of a candidate; 0 = none
    int grp[GT];                        // its group
    int lead[GT];                       // the candidate that represents its group (itself: a leader)
    int rank[GT];                       // a leader's rank among the leaders = the group's output slot
};

// One workgroup per row, one thread per candidate, rank by counting as made_topk_merge does (comparisons only).  A candidate's key
// is what made_group_topw compares -- (score key, lowest column first) -- so the best member of a group is its representative, the
// leaders in descending key order are made_topk_groups_masked's groups, and a member's rank inside its group is its window slot.
// The output row is assembled in LDS (the -1 / -inf fill first), then stored with contiguous writes.
__global__ __launch_bounds__(GT) void topk_candidates_kernel(const int32_t* cand_col, const float* cand_score, int R, const int32_t* col_group,
                                                             int N, int G, int K, int w, int32_t* out_col, float* out_score) {
    extern __shared__ uint32_t v[];                              // [K * w] columns, then [K * w] score bits
    __shared__ CandShared sh;
    const int64_t row = blockIdx.x;
    const int i = threadIdx.x;
    const int KW = K * w;
    uint64_t k = 0ull;
    int g = -1, c = -1;
    if (i < R) {
        c = cand_col[row * R + i];
        if (c >= 0 && c < N) {
            g = col_group ? col_group[c] : c;
            if (col_group && (unsigned)g >= (unsigned)G) g = -1;   // (a column of no group is no item, as in made_topk_groups)
            else k = ((uint64_t)score_key(cand_score[row * R + i]) << 32) | (uint32_t)(0x7FFFFFFF - c);
        }
    }
    sh.key[i] = k; sh.grp[i] = g;
    for (int x = i; x < KW; x += GT) { v[x] = 0xFFFFFFFFu; v[KW + x] = 0xFF800000u; }
    __syncthreads();
    int wr = 0, lead = i;
    if (k != 0ull) {
        uint64_t bk = k;
        for (int q = 0; q < R; ++q) {
            const uint64_t kq = sh.key[q];
            if (kq == 0ull || sh.grp[q] != g) continue;
            wr += (kq > k || (kq == k && q < i)) ? 1 : 0;         // (equal keys -- a column listed twice -- rank in list order)
            if (kq > bk || (kq == bk && q < lead)) { bk = kq; lead = q; }
        }
    }
    sh.lead[i] = lead;
    __syncthreads();
    if (k != 0ull && lead == i) {
        int rk = 0;
        for (int q = 0; q < R; ++q) {
            const uint64_t kq = sh.key[q];
            if (kq == 0ull || sh.lead[q] != q) continue;
            rk += (kq > k || (kq == k && q < i)) ? 1 : 0;
        }
        sh.rank[i] = rk;
    }
    __syncthreads();
    if (k != 0ull) {
        const int slot = sh.rank[lead];
        if (slot < K && wr < w) {
            v[slot * w + wr] = (uint32_t)c;
            v[KW + slot * w + wr] = __float_as_uint(key_score((uint32_t)(k >> 32)));
        }
    }
    __syncthreads();
    for (int x = i; x < KW; x += GT) {
        out_col[row * KW + x] = (int32_t)v[x];
        out_score[row * KW + x] = __uint_as_float(v[KW + x]);
    }
}

}  // namespace

extern "C" int made_topk_candidates(const int32_t* cand_col, const float* cand_score, int64_t Nv, int64_t R, const int32_t* col_group,
                                    int64_t N, int64_t n_groups, int64_t K, int64_t w, int32_t* out_col, float* out_score, void* stream) {
    MADE_REQUIRE(cand_col && cand_score && out_col && out_score, "made_topk_candidates: null pointer");
    MADE_REQUIRE(R >= 1 && R <= GT, "made_topk_candidates: R must lie in [1, 256]");
    MADE_REQUIRE(K >= 1 && K <= 256, "made_topk_candidates: K must lie in [1, 256]");
    MADE_REQUIRE(w >= 1 && w <= 16, "made_topk_candidates: w must lie in [1, 16]");
    MADE_REQUIRE(Nv >= 0 && Nv < (1LL << 31) && N > 0 && N < (1LL << 31), "made_topk_candidates: bad dims (0 <= Nv < 2^31, 0 < N < 2^31)");
    if (col_group) MADE_REQUIRE(n_groups >= 1 && n_groups < (1LL << 31), "made_topk_candidates: n_groups must lie in [1, 2^31)");
    const int64_t nc = Nv * R * 4, no = Nv * K * w * 4;
    MADE_REQUIRE((const void*)out_col != (const void*)out_score && !overlaps(out_col, no, out_score, no) && !overlaps(out_col, no, cand_col, nc) &&
                 !overlaps(out_col, no, cand_score, nc) && !overlaps(out_score, no, cand_col, nc) && !overlaps(out_score, no, cand_score, nc),
                 "made_topk_candidates: the outputs must not alias the inputs or each other");
    if (Nv == 0) return MADE_OK;
    hipLaunchKernelGGL(topk_candidates_kernel, dim3((unsigned)Nv), dim3(GT), (size_t)(K * w * 8), (hipStream_t)stream, cand_col, cand_score, (int)R,
                       col_group, (int)N, (int)n_groups, (int)K, (int)w, out_col, out_score);
    return made_check_launch("made_topk_candidates");
}

extern "C" int made_gather_pairs(const int32_t* vi, const int32_t* mi, int64_t P, int64_t Nv, int64_t Nm,
                                 const void* v_tok, int64_t v_tok_stride, const float* v_mask, int64_t v_mask_stride,
                                 const float* v_vec, int64_t v_vec_stride,
                                 const void* m_tok, int64_t m_tok_stride, const float* m_mask, int64_t m_mask_stride,
                                 const float* m_vec, int64_t m_vec_stride, int64_t Tv, int64_t Ta, int64_t D, int32_t dtype,
                                 void* frame_out, int64_t frame_out_stride, void* seg_out, int64_t seg_out_stride,
                                 float* fmask_out, float* smask_out, float* video_out, float* music_out, void* stream) {
    MADE_REQUIRE(vi && mi && v_tok && v_mask && v_vec && m_tok && m_mask && m_vec && frame_out && seg_out && fmask_out && smask_out &&
                 video_out && music_out, "made_gather_pairs: null pointer");
    MADE_REQUIRE(dtype == MADE_F32 || dtype == MADE_BF16, "made_gather_pairs: dtype must be MADE_F32 or MADE_BF16");
    MADE_REQUIRE(P >= 0 && Nv >= 0 && Nm >= 0 && Tv >= 1 && Ta >= 1 && D >= 1 && P < (1LL << 31), "made_gather_pairs: bad dims");
    const int64_t esz = dtype == MADE_F32 ? 4 : 2;
    MADE_REQUIRE(v_tok_stride >= Tv * D && m_tok_stride >= Ta * D && frame_out_stride >= Tv * D && seg_out_stride >= Ta * D &&
                 v_mask_stride >= Tv && m_mask_stride >= Ta && v_vec_stride >= D && m_vec_stride >= D,
                 "made_gather_pairs: a per-item stride is shorter than the item");
    MADE_REQUIRE((D * esz) % 16 == 0 && (v_tok_stride * esz) % 16 == 0 && (m_tok_stride * esz) % 16 == 0 &&
                 (frame_out_stride * esz) % 16 == 0 && (seg_out_stride * esz) % 16 == 0 && aligned16(v_tok) && aligned16(m_tok) &&
                 aligned16(frame_out) && aligned16(seg_out), "made_gather_pairs: token rows and strides must be 16-byte aligned");
    if (P == 0) return MADE_OK;
    const int64_t s16 = 16 / esz;
    hipLaunchKernelGGL(gather_pairs_kernel, dim3((unsigned)P), dim3(256), 0, (hipStream_t)stream, vi, mi, Nv, Nm,
                       (const uint4*)v_tok, v_tok_stride / s16, v_mask, v_mask_stride, v_vec, v_vec_stride,
                       (const uint4*)m_tok, m_tok_stride / s16, m_mask, m_mask_stride, m_vec, m_vec_stride, (int)Tv, (int)Ta, (int)D,
                       Tv * D / s16, Ta * D / s16, (uint4*)frame_out, frame_out_stride / s16, (uint4*)seg_out, seg_out_stride / s16,
                       fmask_out, smask_out, video_out, music_out);
    return made_check_launch("made_gather_pairs");
}
