// Similar tracks: the top-k cosine neighbours of query rows over a vector table (made_cosine_topk; mgsv_amd/similar.py).  The tile
// loop of made_cosine_join (dedup.hip) with a top-k epilogue instead of a threshold epilogue, and the node semantics of the selection
// kernels: a node (a labelled group, a track with windows, or the column itself) is ranked by its best column and appears once.  The
// reference has no counterpart.
//
// Stage 1, cosine_topk_kernel: one workgroup of 256 threads (4 waves, 2 x 2) takes 128 query rows and walks the 128-column tiles of
// its column split.  The K loop is dedup.hip's, copied: slabs of 32 of the 128 query rows and the 128 table rows go through LDS as
// [256][32 + 4] f32, one slab ahead in registers; a wave owns 2 x 2 accumulator tiles of v_mfma_f32_32x32x2_f32 and a dot product is
// ONE fmaf chain over k in the order 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ...; thread t sums the squares of staged row t in four chains,
// (c0 + c1) + (c2 + c3).  The epilogue divides (one f32 product of the norms, one f32 division), so a (query row, table row) pair has
// the bits made_cosine_join gives the same two rows, whatever Q, N, the splits, or the pair's place in a tile.
//
// The top-k epilogue runs in two passes of 64 columns (accumulator column j = pass of every wave: local column l of a pass is table
// column C + 64 (l >> 5) + 32 pass + (l & 31)), so that the cosines of a pass fit where the staging slabs were: [128][64 + 8] f32,
// the pad puts the two lane halves of a store 32 banks apart.  A cosine whose product of norms is not finite and > 0 is stored as
// NaN.  Then every wave filters its 32 rows (w, w + 4, ...): one candidate per lane against the row's current k-th entry (two broadcast LDS reads),
// one ballot; after the first few tiles almost no row has a survivor.  A row with survivors loads its sorted list (one entry per
// lane, k <= 64) into registers with the entries' nodes and the wave inserts the survivors one by one: an entry of the candidate's
// node is replaced if the candidate is better and keeps its place otherwise, the rest is a ballot for the position and a shift by one
// lane; when more than k candidates survive at once (a split's first tiles) they are first thinned by ranking them among
// themselves.  The order is total -- score descending through the order-preserving key, then column ascending -- so the list after
// a tile does not depend on the order of insertion.  Lists: [128][KL] (cos, col) in LDS, KL = 32 (k <= 32: 70 KB, two workgroups per
// CU) or 64 (102 KB, one).
//
// Stage 2, cosine_topk_merge_kernel: a wave per query folds the splits' partial lists ([splits, Q, k] of (cos, col) in the workspace)
// through the same filter and insertion.  Both stages apply the same total order and node rule, and a node of the final top k is in
// the top k of the split that holds its best column, so the result is bit-identical for every number of splits.  No atomics, no
// inline assembly.
//
// made_cosine_topk_ex adds two things to stage 1, both template parameters of its kernels.  MASK: made_eligibility's bit matrix, one
// row per query -- a column whose bit is clear is no candidate (one more term in the filter's `ok`; the merge never sees such a
// column, so it needs no mask).  And a second first-stage kernel, cosine_topk_narrow_kernel, for few queries: 32 query rows per
// workgroup (below).  The per-row filter, thinning and insertion are one function, kt_offer, that both kernels end in.
#include "common.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int KT_T = 256;                // threads
constexpr int KT_BM = 128;               // tile edge
constexpr int KT_KS = 32;                // slab depth
constexpr int KT_LD = KT_KS + 4;         // LDS row stride of a slab (floats)
constexpr int KT_CS = 64 + 8;            // LDS row stride of a pass's cosines (floats): 128 x 72 = 256 x 36, the slabs' floats
constexpr int KT_CHIP = 512;             // workgroups the launcher's choice of splits aims at (two on each CU of an MI355X)

struct KtEntry {                         // the workspace's element
    float cos;
    int32_t col;
};

// lane l's entry of a sorted list: col < 0 is an empty slot (it ranks below every entry)
struct KtSlot {
    float c;
    int32_t col, nd;
};

__device__ __forceinline__ bool kt_beats(uint32_t ka, int32_t ca, uint32_t kb, int32_t cb) { return ka > kb || (ka == kb && ca < cb); }
__device__ __forceinline__ uint32_t kt_key(float c, int32_t col) { return col < 0 ? 0u : score_key(c); }
__device__ __forceinline__ int32_t kt_col(int32_t col) { return col < 0 ? INT_MAX : col; }
__device__ __forceinline__ int32_t kt_lane_i(int32_t v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float kt_lane_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// the list moved by one lane on the DPP path (VALU only; the __shfl spelling goes through the LDS crossbar, three times per insertion):
// wave_shr:1 gives lane l the value of lane l - 1 (lane 0 keeps its own), wave_shl:1 that of lane l + 1 (lane 63 keeps its own)
template <int CTRL> __device__ __forceinline__ int32_t kt_shift_i(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL> __device__ __forceinline__ KtSlot kt_shift(const KtSlot& L) {
    return {__int_as_float(kt_shift_i<CTRL>(__float_as_int(L.c))), kt_shift_i<CTRL>(L.col), kt_shift_i<CTRL>(L.nd)};
}
constexpr int KT_UP = 0x138, KT_DOWN = 0x130;                    // wave_shr:1, wave_shl:1

// one candidate (the same in every lane; never NaN, col >= 0) into the wave's list of k entries
__device__ __forceinline__ void kt_insert(KtSlot& L, float cc, int32_t ccol, int32_t cnd, int k, int lane) {
    const uint32_t ck = score_key(cc);
    uint32_t ek = kt_key(L.c, L.col);
    int32_t ex = kt_col(L.col);
    const uint64_t same = __ballot(L.col >= 0 && L.nd == cnd);
    if (same) {                                                  // the node is listed: the better of the two stays
        const int p = __ffsll((unsigned long long)same) - 1;
        if (!kt_beats(ck, ccol, (uint32_t)kt_lane_i((int32_t)ek, p), kt_lane_i(ex, p))) return;
        KtSlot nx = kt_shift<KT_DOWN>(L);
        if (lane == WAVE - 1) nx = {-INFINITY, -1, -1};
        if (lane >= p) L = nx;
        ek = kt_key(L.c, L.col);
        ex = kt_col(L.col);
    }
    const int pos = __popcll(__ballot(kt_beats(ek, ex, ck, ccol)));    // the entries before the candidate: a prefix of the sorted list
    if (pos >= k) return;
    const KtSlot up = kt_shift<KT_UP>(L);
    if (lane > pos) L = up;
    if (lane == pos) L = {cc, ccol, cnd};
    if (lane >= k) L = {-INFINITY, -1, -1};
}

// every lane's candidate whose bit is set in m, lowest lane first
__device__ __forceinline__ void kt_insert_all(KtSlot& L, uint64_t m, float c, int32_t col, int32_t nd, int k, int lane) {
    while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        kt_insert(L, kt_lane_f(c, b), kt_lane_i(col, b), kt_lane_i(nd, b), k, lane);
    }
}

// More than k candidates at once (a split's first tiles, the merge's first entries): the candidates of m that can still enter a
// list of k -- a candidate beaten by another of its own node is not its node's best, and a candidate beaten by k others that are each
// the best of a different node is not among the k best nodes.  Comparisons only; without nodes every column is its own node.
__device__ __forceinline__ uint64_t kt_thin(uint64_t m, float c, int32_t col, int32_t nd, bool nodes, int k, int lane) {
    const uint32_t key = score_key(c);
    bool lead = (m >> lane) & 1ull;
    if (nodes) {
        for (uint64_t x = m; x; x &= x - 1) {
            const int b = __ffsll((unsigned long long)x) - 1;
            if (kt_lane_i(nd, b) == nd && kt_beats((uint32_t)kt_lane_i((int32_t)key, b), kt_lane_i(col, b), key, col)) lead = false;
        }
    }
    int before = 0;
    for (uint64_t x = __ballot(lead); x; x &= x - 1) {
        const int b = __ffsll((unsigned long long)x) - 1;
        before += kt_beats((uint32_t)kt_lane_i((int32_t)key, b), kt_lane_i(col, b), key, col) ? 1 : 0;
    }
    return __ballot(lead && before < k);
}

// One row of a tile, one candidate per lane (ok: admissible, and eligible under a mask): the filter against the row's k-th entry, the
// thinning and the insertion into the row's list in LDS (lrow_cos / lrow_col [KL]).  Both first-stage kernels end here.
template <int KL>
__device__ __forceinline__ void kt_offer(bool ok, float c, int32_t col, int32_t cn, float* lrow_cos, int32_t* lrow_col,
                                         const int32_t* __restrict__ node, int k, int lane) {
    const float kc = lrow_cos[k - 1];
    const int32_t kcol = lrow_col[k - 1];
    uint64_t m = __ballot(ok && kt_beats(score_key(c), col, kt_key(kc, kcol), kt_col(kcol)));
    if (!m) return;
    if (__popcll(m) > k) m = kt_thin(m, c, col, cn, node != nullptr, k, lane);
    KtSlot L = {-INFINITY, -1, -1};
    if (lane < KL) L = {lrow_cos[lane], lrow_col[lane], -1};
    if (L.col >= 0) L.nd = node != nullptr ? node[L.col] : L.col;
    kt_insert_all(L, m, c, col, cn, k, lane);
    if (lane < KL) {
        lrow_cos[lane] = L.c;
        lrow_col[lane] = L.col;
    }
}

constexpr int KT_MW = KT_BM / 32;        // mask words of a row over a tile's columns (a tile starts at a multiple of 128 columns)

template <int KL, bool MASK> constexpr size_t kt_lds_bytes() {
    return (size_t)(2 * KT_BM * KT_LD + 2 * KT_BM) * 4 + 2 * KT_BM * 4 + (size_t)KT_BM * KL * 8 + (MASK ? (size_t)KT_BM * KT_MW * 4 : 0);
}

// MASK: bits [Q, bits_ld] is made_eligibility's matrix (column c = bit c & 31 of word c >> 5); a column whose bit is clear in the
// query's row is no candidate.  A tile's words go through LDS ([128][4], loaded with the tile's first slab).
// (under the mask the allocator is held to two waves per SIMD at D = 256 / 512, as the unmasked instantiations reach by themselves: left
// alone it takes 180 + 80 registers, two more than a CU's second workgroup allows; held, 244, no scratch.  The unmasked ones are not touched.)
template <int D, int KL, bool MASK>
__global__ __launch_bounds__(KT_T) __attribute__((amdgpu_waves_per_eu((MASK && D > 128) ? 2 : 1))) void cosine_topk_kernel(const float* __restrict__ query, int64_t Q, const int32_t* __restrict__ query_node,
                                                           const float* __restrict__ vec, int64_t N, const int32_t* __restrict__ node,
                                                           const uint32_t* __restrict__ bits, int64_t bits_ld, int k, int n_row_blocks,
                                                           int n_splits, KtEntry* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kt_smem[];
    float* tile = reinterpret_cast<float*>(kt_smem);             // the slabs: rows 0 .. 127 the queries, 128 .. 255 the table rows; then a pass's cosines
    float* norm = tile + 2 * KT_BM * KT_LD;                      // [256]
    int32_t* cnode = reinterpret_cast<int32_t*>(norm + 2 * KT_BM);      // [128] the tile's column nodes (-1: ignored, or past N)
    int32_t* qnode = cnode + KT_BM;                              // [128] the rows' excluded nodes (-1: none)
    float* lcos = reinterpret_cast<float*>(qnode + KT_BM);       // [128][KL]
    int32_t* lcol = reinterpret_cast<int32_t*>(lcos + KT_BM * KL);      // [128][KL]
    uint32_t* lmask = reinterpret_cast<uint32_t*>(lcol + KT_BM * KL);   // [128][4] (MASK)

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wr = w >> 1, wc = w & 1, r = lane & 31, hh = lane >> 5;
    const int64_t R = (int64_t)(blockIdx.x % (unsigned)n_row_blocks) * KT_BM;
    const int split = (int)(blockIdx.x / (unsigned)n_row_blocks);
    const int64_t rend = R + KT_BM < Q ? R + KT_BM : Q;
    const int64_t n_tiles = (N + KT_BM - 1) / KT_BM;
    const int64_t t0 = n_tiles * split / n_splits, t1 = n_tiles * (split + 1) / n_splits;

    for (int x = tid; x < KT_BM * KL; x += KT_T) {
        lcos[x] = -INFINITY;
        lcol[x] = -1;
    }
    if (tid < KT_BM) {
        const int64_t g = R + tid;
        const int32_t qn = (query_node != nullptr && g < rend) ? query_node[g] : -1;
        qnode[tid] = qn < 0 ? -1 : qn;
    }

    // this thread's eight 16-byte chunks of a slab: staged row q >> 3 (8 chunks per row), chunk q & 7, q = tid + 256 t; t < 4 are query rows
    const float* qsrc[4];
    bool qlive[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = tid + KT_T * t, row = q >> 3;
        qlive[t] = R + row < rend;
        qsrc[t] = query + (qlive[t] ? R + row : R) * D + 4 * (q & 7);
    }

    for (int64_t tt = t0; tt < t1; ++tt) {
        const int64_t C = tt * KT_BM;
        const int64_t cend = C + KT_BM < N ? C + KT_BM : N;
        uint32_t my_mask[2] = {0u, 0u};                          // words tid and tid + 256 of the tile's [128][4]: row x >> 2, word x & 3
        if constexpr (MASK) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int x = tid + KT_T * t, row = x >> 2, wq = x & 3;
                if (R + row < rend && C + 32 * wq < cend) my_mask[t] = bits[(R + row) * bits_ld + (C >> 5) + wq];
            }
            __syncthreads();                                     // the tile before's filter has read its words.  Loaded and stored ahead
            lmask[tid] = my_mask[0];                             // of the slabs' loads, the words and their addresses hold no register
            lmask[tid + KT_T] = my_mask[1];                      // beside those: a dozen more cost a CU its second workgroup (D 256 / 512)
        }

        const float* src[8];
        bool live[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            src[t] = qsrc[t];
            live[t] = qlive[t];
        }
#pragma unroll
        for (int t = 4; t < 8; ++t) {
            const int q = tid + KT_T * t, row = (q >> 3) - KT_BM;
            live[t] = C + row < cend;
            src[t] = vec + (live[t] ? C + row : C) * D + 4 * (q & 7);
        }
        f32x4 pre[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) pre[t] = keep_or_zero(*reinterpret_cast<const f32x4*>(src[t]), live[t]);
        int32_t my_cnode = -1;                                   // the node of column C + tid (stored after the K loop: the tile before's may still be read)
        if (tid < KT_BM && C + tid < cend) my_cnode = node != nullptr ? node[C + tid] : (int32_t)(C + tid);
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;            // squared norm of staged row tid

        for (int s = 0; s < D / KT_KS; ++s) {
            __syncthreads();                                     // the slab before, or the tile before's cosines, have been read
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int q = tid + KT_T * t;
                *reinterpret_cast<f32x4*>(tile + (q >> 3) * KT_LD + 4 * (q & 7)) = pre[t];
            }
            __syncthreads();
            if (s + 1 < D / KT_KS) {
#pragma unroll
                for (int t = 0; t < 8; ++t) pre[t] = keep_or_zero(*reinterpret_cast<const f32x4*>(src[t] + (s + 1) * KT_KS), live[t]);
            }
#pragma unroll
            for (int f = 0; f < KT_KS / 4; ++f) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(tile + tid * KT_LD + 4 * f);
                n0 = fmaf(x[0], x[0], n0);
                n1 = fmaf(x[1], x[1], n1);
                n2 = fmaf(x[2], x[2], n2);
                n3 = fmaf(x[3], x[3], n3);
            }
#pragma unroll
            for (int ks = 0; ks < KT_KS / 8; ++ks) {
                f32x4 a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = *reinterpret_cast<const f32x4*>(tile + (wr * 64 + t * 32 + r) * KT_LD + 8 * ks + 4 * hh);
                    b[t] = *reinterpret_cast<const f32x4*>(tile + (KT_BM + wc * 64 + t * 32 + r) * KT_LD + 8 * ks + 4 * hh);
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
            norm[tid] = (sq > 0.f && sq < INFINITY) ? sqrtf(sq) : 0.f;                // 0: the row has no neighbours
            if (tid < KT_BM) cnode[tid] = my_cnode < 0 ? -1 : my_cnode;
        }

#pragma unroll
        for (int j = 0; j < 2; ++j) {                            // pass j: accumulator column j of every wave
            __syncthreads();                                     // the last slab, or pass 0's cosines, have been read; the norms are written
            const float nb = norm[KT_BM + wc * 64 + j * 32 + r];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = wr * 64 + i * 32 + acc_row(e, hh);
                    const float den = norm[row] * nb;
                    const float c = acc[i][j][e] / den;
                    tile[row * KT_CS + wc * 32 + r] = (den > 0.f && den < INFINITY) ? c : __uint_as_float(0x7FC00000u);
                }
            __syncthreads();
            // this lane's column of the pass, for every row of the wave (rows w, w + 4, ...)
            const int lc = (lane >> 5) * 64 + j * 32 + (lane & 31);
            const int32_t col = (int32_t)(C + lc), cn = cnode[lc];
            for (int i = 0; i < 32; ++i) {
                const int row = 4 * i + w;                       // dealt over the waves: a short block of queries keeps all four busy
                if (R + row >= rend) break;                      // (wave-uniform)
                const float c = tile[row * KT_CS + lane];
                bool ok = c == c && cn >= 0 && cn != qnode[row];
                if constexpr (MASK) ok = ok && ((lmask[row * KT_MW + (lc >> 5)] >> (lc & 31)) & 1u);
                kt_offer<KL>(ok, c, col, cn, lcos + row * KL, lcol + row * KL, node, k, lane);
            }
        }
    }

    // the wave's rows: their lists to the workspace (a wave reads only what it wrote itself)
    for (int i = 0; i < 32; ++i) {
        const int row = 4 * i + w;
        if (R + row >= rend) break;
        if (lane < k) {
            KtEntry en = {lcos[row * KL + lane], lcol[row * KL + lane]};
            part[((int64_t)split * Q + (R + row)) * k + lane] = en;
        }
    }
}

// The 32-row form, for few queries.  A workgroup takes 32 query rows -- one row block of v_mfma_f32_32x32x2_f32 -- so a single query
// pays for 32 rows of products, not 128.  The rows are staged once for the whole walk ([32][D + 4] f32 in LDS, their norms beside
// them); only the table's slabs ([128][32 + 4]) go through LDS per tile, two slabs ahead in registers and across tile ends, so the
// loads of the next tile are in flight during a tile's epilogue.  Wave w owns columns 32 w .. 32 w + 31 of a tile: one accumulator,
// lane (r, hh) holds components 8 ks + 4 hh + e of query row r and of table row 32 w + r and issues e = 0 .. 3 -- the chain, the
// instruction and the operand layout of the 128-row form, and the same four-chain sums of squares, product and division, so a pair
// has the same bits.  The cosines of the tile ([32][128 + 8], where the slabs were) are offered in two halves of 64 columns.
constexpr int KN_BM = 32;                // query rows of a workgroup
constexpr int KN_CS = KT_BM + 8;         // LDS row stride of a tile's cosines (floats): 32 x 136 <= 128 x 36

template <int D, int KL, bool MASK> constexpr size_t kn_lds_bytes() {
    return (size_t)(KN_BM * (D + 4) + KT_BM * KT_LD + KT_BM + KN_BM) * 4 + (size_t)(KT_BM + KN_BM) * 4 + (size_t)KN_BM * KL * 8 +
           (MASK ? (size_t)KN_BM * KT_MW * 4 : 0);
}

template <int D, int KL, bool MASK>
__global__ __launch_bounds__(KT_T) void cosine_topk_narrow_kernel(const float* __restrict__ query, int64_t Q,
                                                                  const int32_t* __restrict__ query_node, const float* __restrict__ vec,
                                                                  int64_t N, const int32_t* __restrict__ node,
                                                                  const uint32_t* __restrict__ bits, int64_t bits_ld, int k, int n_row_blocks,
                                                                  int n_splits, KtEntry* __restrict__ part) {
    constexpr int QLD = D + 4, S = D / KT_KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char kt_smem[];
    float* qs = reinterpret_cast<float*>(kt_smem);               // [32][D + 4] the query rows, staged once
    float* tile = qs + KN_BM * QLD;                              // [128][36] a slab of the table rows; then the tile's cosines [32][136]
    float* norm = tile + KT_BM * KT_LD;                          // [128] the tile's table rows
    float* qnorm = norm + KT_BM;                                 // [32]
    int32_t* cnode = reinterpret_cast<int32_t*>(qnorm + KN_BM);  // [128]
    int32_t* qnode = cnode + KT_BM;                              // [32]
    float* lcos = reinterpret_cast<float*>(qnode + KN_BM);       // [32][KL]
    int32_t* lcol = reinterpret_cast<int32_t*>(lcos + KN_BM * KL);      // [32][KL]
    uint32_t* lmask = reinterpret_cast<uint32_t*>(lcol + KN_BM * KL);   // [32][4] (MASK)

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int64_t R = (int64_t)(blockIdx.x % (unsigned)n_row_blocks) * KN_BM;
    const int split = (int)(blockIdx.x / (unsigned)n_row_blocks);
    const int64_t rend = R + KN_BM < Q ? R + KN_BM : Q;
    const int64_t n_tiles = (N + KT_BM - 1) / KT_BM;
    const int64_t t0 = n_tiles * split / n_splits, t1 = n_tiles * (split + 1) / n_splits;

    // this thread's four 16-byte chunks of a table slab: staged row q >> 3, chunk q & 7, q = tid + 256 t
    auto fetch = [&](int64_t tt, int s, f32x4 (&p)[4]) {
        const int64_t C = tt * KT_BM;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int q = tid + KT_T * t, row = q >> 3;
            const bool live = tt < t1 && C + row < N;
            p[t] = keep_or_zero(*reinterpret_cast<const f32x4*>(vec + (live ? C + row : 0) * D + s * KT_KS + 4 * (q & 7)), live);
        }
    };
    f32x4 pa[4], pb[4];
    fetch(t0, 0, pa);
    fetch(t0, 1, pb);

    for (int x = tid; x < KN_BM * KL; x += KT_T) {
        lcos[x] = -INFINITY;
        lcol[x] = -1;
    }
    if (tid < KN_BM) {
        const int64_t g = R + tid;
        const int32_t qn = (query_node != nullptr && g < rend) ? query_node[g] : -1;
        qnode[tid] = qn < 0 ? -1 : qn;
    }
    for (int x = tid; x < KN_BM * (D / 4); x += KT_T) {
        const int row = x / (D / 4), ch = x % (D / 4);
        const bool live = R + row < rend;
        *reinterpret_cast<f32x4*>(qs + row * QLD + 4 * ch) =
            keep_or_zero(*reinterpret_cast<const f32x4*>(query + (live ? R + row : R) * D + 4 * ch), live);
    }
    __syncthreads();
    if (tid < KN_BM) {                                           // squared norm of query row tid: the four chains of the 128-row form
        float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;
        for (int f = 0; f < D / 4; ++f) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(qs + tid * QLD + 4 * f);
            n0 = fmaf(x[0], x[0], n0);
            n1 = fmaf(x[1], x[1], n1);
            n2 = fmaf(x[2], x[2], n2);
            n3 = fmaf(x[3], x[3], n3);
        }
        const float sq = (n0 + n1) + (n2 + n3);
        qnorm[tid] = (sq > 0.f && sq < INFINITY) ? sqrtf(sq) : 0.f;
    }

    for (int64_t tt = t0; tt < t1; ++tt) {
        const int64_t C = tt * KT_BM;
        const int64_t cend = C + KT_BM < N ? C + KT_BM : N;
        int32_t my_cnode = -1;
        if (tid < KT_BM && C + tid < cend) my_cnode = node != nullptr ? node[C + tid] : (int32_t)(C + tid);
        uint32_t my_mask = 0u;                                   // word tid of the tile's [32][4]: row tid >> 2, word tid & 3
        if constexpr (MASK) {
            const int row = tid >> 2, wq = tid & 3;
            if (tid < KN_BM * KT_MW && R + row < rend && C + 32 * wq < cend) my_mask = bits[(R + row) * bits_ld + (C >> 5) + wq];
        }

        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f;            // squared norm of table row tid of the tile (tid < 128)

        auto step = [&](int s, f32x4 (&p)[4]) {
            __syncthreads();                                     // the slab before, or the tile before's cosines, have been read
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int q = tid + KT_T * t;
                *reinterpret_cast<f32x4*>(tile + (q >> 3) * KT_LD + 4 * (q & 7)) = p[t];
            }
            __syncthreads();
            if (s + 2 < S) fetch(tt, s + 2, p);                  // two slabs ahead; past the tile's end, the next tile's
            else fetch(tt + 1, s + 2 - S, p);
            if (tid < KT_BM) {
#pragma unroll
                for (int f = 0; f < KT_KS / 4; ++f) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(tile + tid * KT_LD + 4 * f);
                    n0 = fmaf(x[0], x[0], n0);
                    n1 = fmaf(x[1], x[1], n1);
                    n2 = fmaf(x[2], x[2], n2);
                    n3 = fmaf(x[3], x[3], n3);
                }
            }
#pragma unroll
            for (int ks = 0; ks < KT_KS / 8; ++ks) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(qs + r * QLD + s * KT_KS + 8 * ks + 4 * hh);
                const f32x4 b = *reinterpret_cast<const f32x4*>(tile + (w * 32 + r) * KT_LD + 8 * ks + 4 * hh);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
            }
        };
        for (int s = 0; s < S; s += 2) {
            step(s, pa);
            step(s + 1, pb);
        }

        if (tid < KT_BM) {
            const float sq = (n0 + n1) + (n2 + n3);
            norm[tid] = (sq > 0.f && sq < INFINITY) ? sqrtf(sq) : 0.f;
            cnode[tid] = my_cnode < 0 ? -1 : my_cnode;
            if constexpr (MASK) lmask[tid] = my_mask;
        }
        __syncthreads();                                         // the last slab has been read; the norms are written
        {
            const float nb = norm[w * 32 + r];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = acc_row(e, hh);
                const float den = qnorm[row] * nb;
                const float c = acc[e] / den;
                tile[row * KN_CS + w * 32 + r] = (den > 0.f && den < INFINITY) ? c : __uint_as_float(0x7FC00000u);
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int lc = 64 * h + lane;                        // this lane's column of the half, for every row of the wave
            const int32_t col = (int32_t)(C + lc), cn = cnode[lc];
            for (int i = 0; i < KN_BM / 4; ++i) {
                const int row = 4 * i + w;
                if (R + row >= rend) break;                      // (wave-uniform)
                const float c = tile[row * KN_CS + lc];
                bool ok = c == c && cn >= 0 && cn != qnode[row];
                if constexpr (MASK) ok = ok && ((lmask[row * KT_MW + (lc >> 5)] >> (lc & 31)) & 1u);
                kt_offer<KL>(ok, c, col, cn, lcos + row * KL, lcol + row * KL, node, k, lane);
            }
        }
    }

    for (int i = 0; i < KN_BM / 4; ++i) {                        // the wave's rows: their lists to the workspace
        const int row = 4 * i + w;
        if (R + row >= rend) break;
        if (lane < k) {
            KtEntry en = {lcos[row * KL + lane], lcol[row * KL + lane]};
            part[((int64_t)split * Q + (R + row)) * k + lane] = en;
        }
    }
}

// a wave per query: the partial lists of every split through the same filter and insertion
__global__ __launch_bounds__(KT_T) void cosine_topk_merge_kernel(const KtEntry* __restrict__ part, int64_t Q, int n_splits, int k,
                                                                 const int32_t* __restrict__ node, int32_t* __restrict__ out_col,
                                                                 float* __restrict__ out_cos) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (KT_T / WAVE) + (threadIdx.x >> 6);
    if (q >= Q) return;                                          // (wave-uniform; no barrier below)
    KtSlot L = {-INFINITY, -1, -1};
    const int total = n_splits * k;
    for (int e0 = 0; e0 < total; e0 += WAVE) {
        const int e = e0 + lane;
        KtEntry en = {-INFINITY, -1};
        if (e < total) en = part[((int64_t)(e / k) * Q + q) * k + (e % k)];
        const int32_t nd = en.col >= 0 ? (node != nullptr ? node[en.col] : en.col) : -1;
        const uint32_t ek = kt_key(L.c, L.col);
        const int32_t ex = kt_col(L.col);
        const uint32_t kk = (uint32_t)kt_lane_i((int32_t)ek, k - 1);
        const int32_t kx = kt_lane_i(ex, k - 1);
        uint64_t m = __ballot(en.col >= 0 && en.cos == en.cos && kt_beats(score_key(en.cos), en.col, kk, kx));
        if (__popcll(m) > k) m = kt_thin(m, en.cos, en.col, nd, node != nullptr, k, lane);
        kt_insert_all(L, m, en.cos, en.col, nd, k, lane);
    }
    if (lane < k) {
        out_col[q * k + lane] = L.col;
        out_cos[q * k + lane] = L.col >= 0 ? L.c : -INFINITY;
    }
}

constexpr int KT_FORM_AUTO = 0, KT_FORM_WIDE = 1, KT_FORM_NARROW = 2;
// form 0: the 32-row form up to this many queries, the 128-row form above.  Measured (README, "Similar tracks"; tools/knn_serving_bench.py):
// at Q = 1, 8, 32, 64 and 128 the 32-row form was faster than the 128-row form at 32 768 and at 400 000 columns by more than the
// run's spread (1.2x - 3.1x); 128 is the largest Q measured, nothing above it was.
constexpr int64_t KN_AUTO_Q = 128;

int topk_form(int64_t Q, int32_t form) { return form != KT_FORM_AUTO ? form : (Q <= KN_AUTO_Q ? KT_FORM_NARROW : KT_FORM_WIDE); }

// the splits of a call: what was asked for, else enough to fill the chip while a split keeps a few tiles; never more than the tiles
// (bm: the query rows of a workgroup, 128 or 32; the column tiles are 128 wide in both forms)
int64_t topk_splits(int64_t Q, int64_t N, int32_t n_splits, int64_t bm = KT_BM) {
    const int64_t tiles = (N + KT_BM - 1) / KT_BM, blocks = (Q + bm - 1) / bm;
    if (tiles == 0 || blocks == 0) return 0;
    int64_t s = n_splits;
    if (s <= 0) {
        s = (KT_CHIP + blocks - 1) / blocks;
        const int64_t per = Q >= KT_BM ? 4 : (Q > 16 ? 2 : 1);   // the first tile of a split fills empty lists: costly with many rows
        const int64_t most = tiles / per > 1 ? tiles / per : 1;
        if (s > most) s = most;
    }
    return s < tiles ? s : tiles;
}

template <typename Kernel>
int topk_reserve(Kernel kernel, size_t lds, bool& reserved) {    // (the attribute is per kernel)
    if (lds > 64 * 1024 && !reserved) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            made_set_error("made_cosine_topk: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
            return MADE_ERR_HIP;
        }
        reserved = true;
    }
    return MADE_OK;
}

struct KtArgs {
    const float* query;
    int64_t Q;
    const int32_t* query_node;
    const float* vec;
    int64_t N;
    const int32_t* node;
    const uint32_t* bits;
    int64_t bits_ld;
    int k;
    int64_t splits;
    KtEntry* part;
    hipStream_t stream;
};

template <int D, int KL, bool MASK, bool NARROW>
int cosine_topk_launch(const KtArgs& a) {
    const int64_t bm = NARROW ? KN_BM : KT_BM, blocks = (a.Q + bm - 1) / bm;
    MADE_UNSUPPORTED(blocks * a.splits < (1LL << 31), "made_cosine_topk: %lld row blocks x %lld splits in one call, split the queries",
                     (long long)blocks, (long long)a.splits);
    static bool reserved = false;
    if constexpr (NARROW) {
        constexpr size_t lds = kn_lds_bytes<D, KL, MASK>();
        const auto kernel = cosine_topk_narrow_kernel<D, KL, MASK>;
        if (int rc = topk_reserve(kernel, lds, reserved); rc != MADE_OK) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks * a.splits)), dim3(KT_T), lds, a.stream, a.query, a.Q, a.query_node, a.vec, a.N,
                           a.node, a.bits, a.bits_ld, a.k, (int)blocks, (int)a.splits, a.part);
    } else {
        constexpr size_t lds = kt_lds_bytes<KL, MASK>();
        const auto kernel = cosine_topk_kernel<D, KL, MASK>;
        if (int rc = topk_reserve(kernel, lds, reserved); rc != MADE_OK) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks * a.splits)), dim3(KT_T), lds, a.stream, a.query, a.Q, a.query_node, a.vec, a.N,
                           a.node, a.bits, a.bits_ld, a.k, (int)blocks, (int)a.splits, a.part);
    }
    return made_check_launch("made_cosine_topk");
}

template <int D, bool MASK, bool NARROW>
int cosine_topk_lists(const KtArgs& a) {
    return a.k <= 32 ? cosine_topk_launch<D, 32, MASK, NARROW>(a) : cosine_topk_launch<D, 64, MASK, NARROW>(a);
}

template <int D>
int cosine_topk_form(const KtArgs& a, bool narrow) {
    if (narrow) return a.bits != nullptr ? cosine_topk_lists<D, true, true>(a) : cosine_topk_lists<D, false, true>(a);
    return a.bits != nullptr ? cosine_topk_lists<D, true, false>(a) : cosine_topk_lists<D, false, false>(a);
}

// both entry points: form is 1 or 2 here, bits may be null
int cosine_topk_run(const float* query, int64_t Q, const int32_t* query_node, const float* vec, int64_t N, int64_t D, const int32_t* node,
                    const uint32_t* bits, int64_t bits_ld, int64_t k, int32_t n_splits, int form, int32_t* out_col, float* out_cos, void* ws,
                    int64_t ws_bytes, void* stream) {
    MADE_REQUIRE(Q >= 0 && N >= 0 && n_splits >= 0, "made_cosine_topk: bad dims (Q, N, n_splits >= 0)");
    MADE_UNSUPPORTED(Q < (1LL << 31) && N < (1LL << 31), "made_cosine_topk: Q and N must be < 2^31");
    MADE_UNSUPPORTED(D == 128 || D == 256 || D == 512, "made_cosine_topk: D must be 128, 256 or 512, got %lld", (long long)D);
    MADE_UNSUPPORTED(k >= 1 && k <= 64, "made_cosine_topk: k must be in [1, 64], got %lld", (long long)k);
    if (Q == 0) return MADE_OK;
    MADE_REQUIRE(query != nullptr && out_col != nullptr && out_cos != nullptr && (vec != nullptr || N == 0), "made_cosine_topk: null pointer");
    MADE_REQUIRE(((uintptr_t)query & 15u) == 0 && ((uintptr_t)vec & 15u) == 0, "made_cosine_topk: query and vec must be 16-byte aligned");
    MADE_REQUIRE(bits == nullptr || bits_ld >= (N + 31) / 32, "made_cosine_topk_ex: bits_ld must be >= ceil(N / 32)");
    const bool narrow = form == KT_FORM_NARROW;
    const int64_t splits = topk_splits(Q, N, n_splits, narrow ? KN_BM : KT_BM), need = splits * Q * k * (int64_t)sizeof(KtEntry);
    MADE_UNSUPPORTED(ws_bytes >= need, "made_cosine_topk: the workspace holds %lld bytes, %lld are needed (made_cosine_topk_ws_bytes)",
                     (long long)ws_bytes, (long long)need);
    MADE_REQUIRE(ws != nullptr || need == 0, "made_cosine_topk: null pointer");
    MADE_REQUIRE(((uintptr_t)ws & 7u) == 0, "made_cosine_topk: the workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    KtEntry* part = reinterpret_cast<KtEntry*>(ws);
    if (splits > 0) {
        const KtArgs a = {query, Q, query_node, vec, N, node, bits, bits_ld, (int)k, splits, part, st};
        int rc;
        if (D == 128) rc = cosine_topk_form<128>(a, narrow);
        else if (D == 256) rc = cosine_topk_form<256>(a, narrow);
        else rc = cosine_topk_form<512>(a, narrow);
        if (rc != MADE_OK) return rc;
    }
    const int per = KT_T / WAVE;
    hipLaunchKernelGGL(cosine_topk_merge_kernel, dim3((unsigned)((Q + per - 1) / per)), dim3(KT_T), 0, st, part, Q, (int)splits, (int)k, node,
                       out_col, out_cos);
    return made_check_launch("made_cosine_topk");
}

}  // namespace

extern "C" int64_t made_cosine_topk_ws_bytes(int64_t Q, int64_t N, int64_t k, int32_t n_splits) {
    if (Q < 0 || N < 0 || k < 1 || k > 64 || n_splits < 0 || Q >= (1LL << 31) || N >= (1LL << 31)) return -1;
    return topk_splits(Q, N, n_splits) * Q * k * (int64_t)sizeof(KtEntry);
}

extern "C" int made_cosine_topk(const float* query, int64_t Q, const int32_t* query_node, const float* vec, int64_t N, int64_t D,
                                const int32_t* node, int64_t k, int32_t n_splits, int32_t* out_col, float* out_cos, void* ws, int64_t ws_bytes,
                                void* stream) {
    return cosine_topk_run(query, Q, query_node, vec, N, D, node, nullptr, 0, k, n_splits, KT_FORM_WIDE, out_col, out_cos, ws, ws_bytes, stream);
}

extern "C" int64_t made_cosine_topk_ex_ws_bytes(int64_t Q, int64_t N, int64_t k, int32_t n_splits, int32_t form) {
    if (Q < 0 || N < 0 || k < 1 || k > 64 || n_splits < 0 || Q >= (1LL << 31) || N >= (1LL << 31) || form < 0 || form > 2) return -1;
    return topk_splits(Q, N, n_splits, topk_form(Q, form) == KT_FORM_NARROW ? KN_BM : KT_BM) * Q * k * (int64_t)sizeof(KtEntry);
}

extern "C" int made_cosine_topk_ex(const float* query, int64_t Q, const int32_t* query_node, const float* vec, int64_t N, int64_t D,
                                   const int32_t* node, const uint32_t* bits, int64_t bits_ld, int64_t k, int32_t n_splits, int32_t form,
                                   int32_t* out_col, float* out_cos, void* ws, int64_t ws_bytes, void* stream) {
    MADE_UNSUPPORTED(form >= 0 && form <= 2, "made_cosine_topk_ex: form must be 0 (chosen by the launcher), 1 (128-row tiles) or 2 (32-row tiles), got %d",
                     (int)form);
    return cosine_topk_run(query, Q, query_node, vec, N, D, node, bits, bits_ld, k, n_splits, topk_form(Q, form), out_col, out_cos, ws, ws_bytes,
                           stream);
}
