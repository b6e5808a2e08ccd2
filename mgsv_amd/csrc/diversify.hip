// Diversified grounding: the greedy re-selection of every video's k results among a pool of P >= k selected groups
// (made_mmr_select; grounding.ground(..., diversity= / max_similarity= / pool=)).  A slot's objective is its score minus mu times the
// largest cosine between its vector and the vector of a slot picked before it; a slot whose largest cosine exceeds tau is dropped.
// The reference has no counterpart: it ranks by similarity alone (test-MaDe.py:386-408).
//
// One workgroup of 256 threads per video.  Thread j owns slot j (score, norm, the running maximum m_j, picked / dropped); a ROW
// GROUP of 16 lanes (one DPP row) forms the dot product of one pool row with the row just picked, 16 rows per workgroup at a time.
// Lane s of a row group holds the 16-byte fragments s, s + 16, s + 32, ... of its row, so a row group reads 256 contiguous bytes
// per access.  A dot product is summed in ONE order whatever the rows are read from: per lane four chains (one per component of
// the fragment) over the lane's fragments in ascending order, (c0 + c1) + (c2 + c3), then the DPP tree xor 1, xor 2, ror 4, ror 8
// as lane 0 of the row group sees it.  So the two forms below give the same bits for the same slot:
//   LDS form:    the P rows are gathered once into LDS (P * D * 4 bytes <= MMR_LDS_ROWS) and every step reads them there.  The
//                row stride is D floats, unpadded on purpose: the four row groups of a wave read the same fragment index of four
//                rows, and ds_read_b128 serves lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... together -- with a stride
//                that is a multiple of 64 banks the parts of two rows in one such group cover disjoint banks, with a 16-byte pad
//                they would not.
//   global form: every step reads the rows from the vector table again (a video's rows stay in L2 between its steps).
// No atomics, no inline assembly; every store is an ordinary vector store.
#include "common.h"

#include <math.h>

namespace {

constexpr int MMR_T = 256;                                       // threads = most slots
constexpr int64_t MMR_LDS_ROWS = 144 * 1024;                     // most bytes of gathered rows (the CU has 160 KiB; the rest: MmrAux)

struct MmrAux {
    float dot[MMR_T];                    // a step's dot products (row groups -> slot owners)
    int row[MMR_T];                      // a slot's row of the vector table, -1: absent (never changed after the start)
    int alive[MMR_T];                    // present, not picked, not dropped
    uint64_t wmax[MMR_T / 64];           // the waves' best keys
    float pick_norm;                     // the picked slot's norm
    float pad[3];
};

template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t l = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);      // (lanes a control does not write keep their own)
    const uint32_t h = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return ((uint64_t)h << 32) | l;
}

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// the largest key of the wave, in every lane (common.h's wave_max on 64-bit keys; a maximum does not depend on the order)
__device__ __forceinline__ uint64_t wave_max_key(uint64_t v) {
    v = max_u64(v, dpp_u64<0xB1, 0xF>(v));                       // quad_perm [1,0,3,2]
    v = max_u64(v, dpp_u64<0x4E, 0xF>(v));                       // quad_perm [2,3,0,1]
    v = max_u64(v, dpp_u64<0x124, 0xF>(v));                      // row_ror:4
    v = max_u64(v, dpp_u64<0x128, 0xF>(v));                      // row_ror:8
    v = max_u64(v, dpp_u64<0x142, 0xA>(v));                      // row_bcast:15 -> rows 1, 3
    v = max_u64(v, dpp_u64<0x143, 0xC>(v));                      // row_bcast:31 -> rows 2, 3
    const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63);
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((uint64_t)h << 32) | l;
}

template <int D> struct Frag { f32x4 v[D / 64]; };              // a lane's share of a row: fragments s, s + 16, ...

template <int D> __device__ __forceinline__ Frag<D> load_frag(const float* base, int s) {
    Frag<D> f;
#pragma unroll
    for (int i = 0; i < D / 64; ++i) f.v[i] = *reinterpret_cast<const f32x4*>(base + 4 * (s + 16 * i));
    return f;
}

// the row group's dot product; the value of the group's lane 0 is the one that is used
template <int D> __device__ __forceinline__ float frag_dot(const Frag<D>& a, const Frag<D>& b) {
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
#pragma unroll
    for (int i = 0; i < D / 64; ++i) {
        c0 = fmaf(a.v[i][0], b.v[i][0], c0);
        c1 = fmaf(a.v[i][1], b.v[i][1], c1);
        c2 = fmaf(a.v[i][2], b.v[i][2], c2);
        c3 = fmaf(a.v[i][3], b.v[i][3], c3);
    }
    float v = (c0 + c1) + (c2 + c3);
    v += dpp_f32<0xB1, 0xF>(v, v);
    v += dpp_f32<0x4E, 0xF>(v, v);
    v += dpp_f32<0x124, 0xF>(v, v);
    v += dpp_f32<0x128, 0xF>(v, v);
    return v;
}

// key of an available slot: (objective in the selection's order: NaN lowest, -inf below every number, -0 = +0; the smaller j first)
__device__ __forceinline__ uint64_t slot_key(float obj, int j) { return ((uint64_t)score_key(obj) << 32) | (uint32_t)(MMR_T - 1 - j); }

template <int D, bool LDS>
__global__ __launch_bounds__(MMR_T) void mmr_select_kernel(const int32_t* row, const float* score, const float* vec, int64_t n_rows,
                                                           int P, int k, float mu, float tau, int32_t* pos, float* redundancy) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* rows = reinterpret_cast<float*>(smem);                                    // [P, D] (LDS form)
    MmrAux& sh = *reinterpret_cast<MmrAux*>(smem + (LDS ? (size_t)P * D * 4 : 0));
    const int64_t vid = blockIdx.x;
    const int tid = threadIdx.x;
    const int g = tid >> 4, s = tid & 15;
    const float nan = __uint_as_float(0x7FC00000u);

    int r = -1;
    float sc = 0.f;
    if (tid < P) {
        const int64_t x = row[vid * P + tid];
        r = (x >= 0 && x < n_rows) ? (int)x : -1;
        sc = score[vid * P + tid];
        sh.row[tid] = r;
        sh.alive[tid] = r >= 0;
    }
    __syncthreads();
    // the rows' squared norms (and, LDS form, the rows into LDS)
    for (int j = g; j < P; j += 16) {
        const int rj = sh.row[j];
        if (rj < 0) continue;                                    // (uniform over the row group)
        const Frag<D> a = load_frag<D>(vec + (int64_t)rj * D, s);
        if constexpr (LDS) {
#pragma unroll
            for (int i = 0; i < D / 64; ++i) *reinterpret_cast<f32x4*>(rows + (size_t)j * D + 4 * (s + 16 * i)) = a.v[i];
        }
        const float n2 = frag_dot<D>(a, a);
        if (s == 0) sh.dot[j] = n2;
    }
    __syncthreads();
    float nrm = 0.f;                                             // 0: the cosine with this slot is 0
    if (r >= 0) {
        const float n2 = sh.dot[tid];
        if (n2 > 0.f && n2 < INFINITY) nrm = sqrtf(n2);
    }
    float m = 0.f;                                               // the running maximum (defined after the first pick)
    bool avail = r >= 0;
    uint64_t key = avail ? slot_key(sc, tid) : 0ull;
    int t = 0;
    for (; t < k; ++t) {
        const uint64_t wbest = wave_max_key(key);
        if ((tid & 63) == 0) sh.wmax[tid >> 6] = wbest;
        __syncthreads();                                         // (1): the waves' keys; everything of the step before has been read
        const uint64_t best = max_u64(max_u64(sh.wmax[0], sh.wmax[1]), max_u64(sh.wmax[2], sh.wmax[3]));
        if ((best >> 32) == 0ull) break;                         // nothing is left (uniform)
        const int jp = MMR_T - 1 - (int)(uint32_t)best;
        if (tid == jp) {
            pos[vid * k + t] = jp;
            redundancy[vid * k + t] = t == 0 ? nan : m;
            sh.pick_norm = nrm;
            avail = false;
            key = 0ull;
        }
        if (t + 1 == k) { ++t; break; }
        const Frag<D> p = load_frag<D>(LDS ? rows + (size_t)jp * D : vec + (int64_t)sh.row[jp] * D, s);
        for (int j = g; j < P; j += 16) {
            if (!sh.alive[j] || j == jp) continue;               // (uniform over the row group)
            const Frag<D> a = load_frag<D>(LDS ? rows + (size_t)j * D : vec + (int64_t)sh.row[j] * D, s);
            const float d = frag_dot<D>(a, p);
            if (s == 0) sh.dot[j] = d;
        }
        __syncthreads();                                         // (2): the dot products and the picked slot's norm
        if (tid == jp) sh.alive[jp] = 0;
        if (avail) {
            const float den = nrm * sh.pick_norm;
            float c = 0.f;
            if (den > 0.f && den < INFINITY) c = sh.dot[tid] / den;
            if (c != c) c = 0.f;
            m = t == 0 ? c : fmaxf(m, c);
            if (m > tau) {                                       // dropped for good
                avail = false;
                sh.alive[tid] = 0;
                key = 0ull;
            } else {
                key = slot_key(fmaf(-mu, m, sc), tid);
            }
        }
    }
    for (int x = t + tid; x < k; x += MMR_T) {
        pos[vid * k + x] = -1;
        redundancy[vid * k + x] = nan;
    }
}

bool mmr_overlaps(const void* p, int64_t pn, const void* q, int64_t qn) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return pn > 0 && qn > 0 && a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

template <int D, bool LDS>
int mmr_launch(const int32_t* row, const float* score, const float* vec, int64_t n_rows, int64_t Nv, int64_t P, int64_t k, float mu,
               float tau, int32_t* pos, float* redundancy, hipStream_t stream) {
    const size_t lds = sizeof(MmrAux) + (LDS ? (size_t)(P * D * 4) : 0);
    static size_t allowed = 64 * 1024;                           // (grown in steps; the attribute is per kernel, set before a larger launch)
    if (lds > allowed) {
        hipError_t e = hipFuncSetAttribute((const void*)mmr_select_kernel<D, LDS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(MMR_LDS_ROWS + sizeof(MmrAux)));
        if (e != hipSuccess) {
            made_set_error("made_mmr_select: cannot reserve %zu bytes of LDS: %s", lds, hipGetErrorString(e));
            return MADE_ERR_HIP;
        }
        allowed = MMR_LDS_ROWS + sizeof(MmrAux);
    }
    const auto kernel = mmr_select_kernel<D, LDS>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)Nv), dim3(MMR_T), lds, stream, row, score, vec, n_rows, (int)P, (int)k, mu, tau, pos, redundancy);
    return made_check_launch("made_mmr_select");
}

template <int D>
int mmr_launch_form(bool lds, const int32_t* row, const float* score, const float* vec, int64_t n_rows, int64_t Nv, int64_t P, int64_t k,
                    float mu, float tau, int32_t* pos, float* redundancy, hipStream_t stream) {
    return lds ? mmr_launch<D, true>(row, score, vec, n_rows, Nv, P, k, mu, tau, pos, redundancy, stream)
               : mmr_launch<D, false>(row, score, vec, n_rows, Nv, P, k, mu, tau, pos, redundancy, stream);
}

}  // namespace

extern "C" int made_mmr_select(const int32_t* row, const float* score, const float* vec, int64_t n_rows, int64_t D, int64_t Nv, int64_t P,
                               int64_t k, float mu, float tau, int32_t* pos, float* redundancy, void* stream) {
    MADE_REQUIRE(row && score && pos && redundancy && (vec || n_rows == 0), "made_mmr_select: null pointer");
    MADE_REQUIRE(Nv >= 0 && Nv < (1LL << 31) && n_rows >= 0 && n_rows < (1LL << 31), "made_mmr_select: bad dims (0 <= Nv, n_rows < 2^31)");
    MADE_REQUIRE(P >= 1 && P <= MMR_T && k >= 1 && k <= P, "made_mmr_select: needs 1 <= k <= P <= 256, got k = %lld, P = %lld", (long long)k,
                 (long long)P);
    MADE_REQUIRE(mu >= 0.f && mu < INFINITY, "made_mmr_select: mu must be finite and >= 0");
    MADE_REQUIRE(tau > -1.f, "made_mmr_select: tau must be > -1 (+inf: nothing is dropped)");
    MADE_UNSUPPORTED(D == 128 || D == 256 || D == 512, "made_mmr_select: D must be 128, 256 or 512, got %lld", (long long)D);
    MADE_REQUIRE(((uintptr_t)vec & 15u) == 0, "made_mmr_select: vec must be 16-byte aligned");
    const int64_t ni = Nv * P * 4, no = Nv * k * 4;
    MADE_REQUIRE(!mmr_overlaps(pos, no, redundancy, no) && !mmr_overlaps(pos, no, row, ni) && !mmr_overlaps(pos, no, score, ni) &&
                 !mmr_overlaps(redundancy, no, row, ni) && !mmr_overlaps(redundancy, no, score, ni) &&
                 !mmr_overlaps(pos, no, vec, n_rows * D * 4) && !mmr_overlaps(redundancy, no, vec, n_rows * D * 4),
                 "made_mmr_select: the outputs must not alias the inputs or each other");
    if (Nv == 0) return MADE_OK;
    bool lds = P * D * 4 <= MMR_LDS_ROWS;
    if (const char* form = made_variant_env("MADE_MMR_FORM")) {   // measurements and the form-equality test: "global" re-reads the table
        if (strcmp(form, "global") == 0) lds = false;
    }
    hipStream_t st = (hipStream_t)stream;
    if (D == 128) return mmr_launch_form<128>(lds, row, score, vec, n_rows, Nv, P, k, mu, tau, pos, redundancy, st);
    if (D == 256) return mmr_launch_form<256>(lds, row, score, vec, n_rows, Nv, P, k, mu, tau, pos, redundancy, st);
    return mmr_launch_form<512>(lds, row, score, vec, n_rows, Nv, P, k, mu, tau, pos, redundancy, st);
}
