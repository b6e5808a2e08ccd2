// Batches from a device-resident feature store (mgsv_amd/feature_store.py DeviceFeatureStore): made_gather_batch assembles every
// tensor of a training / evaluation batch -- frame and segment features, their masks, the per-sample tables -- in ONE launch from
// arrays that stay on the device in their storage format (f32, raw bf16, u8 masks), widened to the f32 the step reads.  The
// widening moves bits or converts integers, so a batch holds exactly the values the host loader would have uploaded.  The kernel
// streams: no LDS, no atomics, no workspace.  The reference assembles its batches on the host (dataloader_MGSV_EC_feature.py).
#include "common.h"

namespace {

// the launcher's view of one array: `units` lanes per destination row, each 16 source bytes (vec) or one element
struct GatherArray {
    const void* src;
    const int32_t* row;
    uint32_t* dst;
    int64_t rows;
    uint32_t units;
    int32_t kind;
    int32_t vec;
    uint32_t nb;            // destination rows: B, or 0 for an array without elements
};

struct GatherParams {
    GatherArray a[MADE_GATHER_MAX_ARRAYS];
    const int32_t* index;
    int64_t n_samples;
};

__device__ __forceinline__ uint32_t u8_bits(uint32_t w, int k) { return __float_as_uint((float)((w >> (8 * k)) & 0xFFu)); }

__device__ __forceinline__ uint4 widen_bf16x4(uint32_t a, uint32_t b) {      // element 0 is the low half of a (little endian)
    return make_uint4(a << 16, a & 0xFFFF0000u, b << 16, b & 0xFFFF0000u);
}

__device__ __forceinline__ uint4 widen_u8x4(uint32_t w) { return make_uint4(u8_bits(w, 0), u8_bits(w, 1), u8_bits(w, 2), u8_bits(w, 3)); }

// blockIdx.y = the array (its descriptor is read from the kernel arguments with a uniform index), blockIdx.x * 256 + lane = b * units + u:
// destination row b, piece u.  The launcher keeps B * units below 2^31, so the lane number and its division stay in 32 bits; the
// element offsets are 64-bit (rows * row_elems may pass 2^32).
__global__ __launch_bounds__(256) void gather_batch_kernel(const GatherParams p) {
    const GatherArray& a = p.a[blockIdx.y];
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t b = g / a.units;
    if (b >= a.nb) return;                                       // (also every block past this array's own count)
    const uint32_t u = g - b * a.units;
    const int64_t s = p.index[b];
    int64_t r = -1;
    if (s >= 0 && s < p.n_samples) {
        r = a.row ? (int64_t)a.row[s] : s;
        if (r >= a.rows) r = -1;
    }
    const bool live = r >= 0;                                    // otherwise: a zero row, nothing read
    const int64_t so = r * (int64_t)a.units + u, d = (int64_t)b * a.units + u;
    if (a.vec) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (live) v = ((const uint4*)a.src)[so];
        uint4* dst = (uint4*)a.dst;
        if (a.kind == MADE_GATHER_F32) {
            dst[d] = v;
        } else if (a.kind == MADE_GATHER_BF16) {
            dst[2 * d] = widen_bf16x4(v.x, v.y);
            dst[2 * d + 1] = widen_bf16x4(v.z, v.w);
        } else {
            dst[4 * d] = widen_u8x4(v.x);
            dst[4 * d + 1] = widen_u8x4(v.y);
            dst[4 * d + 2] = widen_u8x4(v.z);
            dst[4 * d + 3] = widen_u8x4(v.w);
        }
    } else {
        uint32_t v = 0u;
        if (live) {
            if (a.kind == MADE_GATHER_F32) v = ((const uint32_t*)a.src)[so];
            else if (a.kind == MADE_GATHER_BF16) v = (uint32_t)((const uint16_t*)a.src)[so] << 16;
            else v = __float_as_uint((float)((const uint8_t*)a.src)[so]);
        }
        a.dst[d] = v;
    }
}

bool aligned_to(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return na > 0 && nb > 0 && x < y + (uintptr_t)nb && y < x + (uintptr_t)na;
}

}  // namespace

extern "C" int made_gather_batch(const MadeGatherBatchArgs* args, void* stream) {
    MADE_REQUIRE(args != nullptr, "made_gather_batch: null args");
    const MadeGatherBatchArgs& g = *args;
    const int64_t lim = 1LL << 31;
    MADE_REQUIRE(g.n_arrays >= 1 && g.n_arrays <= MADE_GATHER_MAX_ARRAYS, "made_gather_batch: n_arrays=%d outside [1, %d]", g.n_arrays,
                 MADE_GATHER_MAX_ARRAYS);
    MADE_REQUIRE(g.B >= 0 && g.B <= lim && g.n_samples >= 0 && g.n_samples <= lim, "made_gather_batch: B=%lld or n_samples=%lld outside [0, 2^31]",
                 (long long)g.B, (long long)g.n_samples);
    if (g.B == 0) return MADE_OK;
    MADE_REQUIRE(g.index != nullptr && aligned_to(g.index, 4), "made_gather_batch: null or misaligned index");
    GatherParams p = {};
    p.index = g.index;
    p.n_samples = g.n_samples;
    int64_t blocks = 0;
    for (int i = 0; i < g.n_arrays; ++i) {
        const MadeGatherArray& a = g.a[i];
        MADE_REQUIRE(a.kind == MADE_GATHER_F32 || a.kind == MADE_GATHER_BF16 || a.kind == MADE_GATHER_U8, "made_gather_batch: array %d: bad kind %d", i,
                     a.kind);
        MADE_REQUIRE(a.rows >= 0 && a.rows <= lim && a.row_elems >= 0, "made_gather_batch: array %d: rows=%lld outside [0, 2^31] or row_elems=%lld < 0", i,
                     (long long)a.rows, (long long)a.row_elems);
        MADE_REQUIRE(a.row_elems < lim && g.B * a.row_elems < lim, "made_gather_batch: array %d: B * row_elems = %lld * %lld too large for one launch",
                     i, (long long)g.B, (long long)a.row_elems);
        const int64_t esz = a.kind == MADE_GATHER_F32 ? 4 : a.kind == MADE_GATHER_BF16 ? 2 : 1;
        MADE_REQUIRE(a.dst != nullptr && (a.src != nullptr || a.rows == 0), "made_gather_batch: array %d: null src or dst", i);
        MADE_REQUIRE(aligned_to(a.src, (uintptr_t)esz) && aligned_to(a.dst, 4) && aligned_to(a.row, 4),
                     "made_gather_batch: array %d: src, row or dst not aligned to its element", i);
        MADE_REQUIRE(!overlap(a.dst, g.B * a.row_elems * 4, a.src, a.rows * a.row_elems * esz), "made_gather_batch: array %d: dst overlaps src", i);
        GatherArray& o = p.a[i];
        o.src = a.src; o.row = a.row; o.dst = (uint32_t*)a.dst; o.rows = a.rows; o.kind = a.kind;
        const int64_t per = 16 / esz;                            // source elements of one 16-byte piece
        o.vec = (a.row_elems % per == 0 && aligned_to(a.src, 16) && aligned_to(a.dst, 16)) ? 1 : 0;
        o.units = (uint32_t)(o.vec ? a.row_elems / per : a.row_elems);
        if (o.units == 0) { o.units = 1; continue; }             // row_elems == 0: nb stays 0, every lane of its blocks leaves
        o.nb = (uint32_t)g.B;
        blocks = std::max(blocks, (g.B * (int64_t)o.units + 255) / 256);
    }
    for (int i = g.n_arrays; i < MADE_GATHER_MAX_ARRAYS; ++i) p.a[i].units = 1;
    if (blocks == 0) return MADE_OK;
    hipLaunchKernelGGL(gather_batch_kernel, dim3((unsigned)blocks, (unsigned)g.n_arrays), dim3(256), 0, (hipStream_t)stream, p);
    return made_check_launch("made_gather_batch");
}
