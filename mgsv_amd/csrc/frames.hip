// Frame preprocessing for the CLIP ViT-B/32 visual tower (mgsv_amd/frames.py): decoded RGB uint8 frames of any size -> the 49
// patch rows of the 224 x 224 centre crop, the A operand of conv1 as a GEMM.  One pass per frame restates torchvision's
// Resize(224, BICUBIC) (PIL's separable resample: horizontal pass first, a uint8 intermediate, 22-bit fixed-point taps),
// CenterCrop(224), ToTensor and CLIP's Normalize (reference dataloaders/dataloader_MGSV_EC_rawdata.py:16-25).  The host computes
// every tap in double exactly as PIL does and bakes the crop into the tables; the kernel does integer multiply-adds only, so the
// crop is bit-identical to PIL's.
#include "common.h"

namespace {

constexpr int S = 224;                  // crop side
constexpr int BAND = 16;                // output rows per workgroup (inside one 32-row patch row)
constexpr int CH = 32;                  // intermediate rows staged in LDS per step: 32 x 224 x 3 bytes = 21 KiB
constexpr int PT = 256;                 // threads: the vertical pass gives thread j < 224 output column j
constexpr int PREC = 22;                // PIL's PRECISION_BITS (32 - 8 - 2)

__device__ __forceinline__ int clip8(int s) {                       // PIL clip8: (s >> 22) clamped to [0, 255]
    const int v = s >> PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// workgroup x: frame x / (S / BAND), band x % (S / BAND).  The coefficient block of a frame (MadeFrameDesc.coef) holds S rows of
// (first input column, tap count, kh taps) for the crop's output columns, then S rows of (first input row, tap count, kv taps) for
// its output rows.  Reads are clamped to the frame and the table (a malformed table cannot leave either); a descriptor that does
// not fit the buffers yields NaN patch rows and a zero crop.
__global__ __launch_bounds__(PT) void frames_preprocess_kernel(const uint8_t* __restrict__ frames, int64_t frames_bytes,
                                                               const MadeFrameDesc* __restrict__ desc, const int32_t* __restrict__ coef,
                                                               int64_t n_coef, void* patches, int dtype, int64_t ldp, uint8_t* crop) {
    __shared__ uint8_t tmp[CH][S * 3];
    const int64_t f = blockIdx.x / (S / BAND);
    const int i0 = (int)(blockIdx.x % (S / BAND)) * BAND;
    const int tid = threadIdx.x;
    const MadeFrameDesc d = desc[f];
    const bool ok = d.H >= 1 && d.W >= 1 && d.kh >= 1 && d.kh <= 255 && d.kv >= 1 && d.kv <= 255 && d.offset >= 0 &&
                    d.offset + (int64_t)3 * d.H * d.W <= frames_bytes && d.coef >= 0 &&
                    d.coef + (int64_t)S * (4 + d.kh + d.kv) <= n_coef;
    int acc[BAND][3];
#pragma unroll
    for (int ii = 0; ii < BAND; ++ii) acc[ii][0] = acc[ii][1] = acc[ii][2] = 1 << (PREC - 1);
    if (ok) {
        const uint8_t* img = frames + d.offset;
        const int32_t* hc = coef + d.coef;
        const int32_t* vc = hc + (int64_t)S * (2 + d.kh);
        // the input rows this band's output rows read
        int y_lo = d.H, y_hi = 0;
        for (int ii = 0; ii < BAND; ++ii) {
            const int32_t* r = vc + (int64_t)(i0 + ii) * (2 + d.kv);
            const int ymin = min(max(r[0], 0), d.H - 1);
            const int n = min(min(max(r[1], 0), d.kv), d.H - ymin);
            y_lo = min(y_lo, ymin);
            y_hi = max(y_hi, ymin + n);
        }
        for (int y0 = y_lo; y0 < y_hi; y0 += CH) {
            const int rows = min(CH, y_hi - y0);
            // horizontal pass of input rows y0 .. y0 + rows - 1, the crop's columns only -> uint8 in LDS
            for (int it = tid; it < rows * S; it += PT) {
                const int r = it / S, j = it - r * S;
                const int32_t* c = hc + (int64_t)j * (2 + d.kh);
                const int xmin = min(max(c[0], 0), d.W - 1);
                const int n = min(min(max(c[1], 0), d.kh), d.W - xmin);
                const uint8_t* p = img + ((int64_t)(y0 + r) * d.W + xmin) * 3;
                int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
                for (int t = 0; t < n; ++t) {
                    const int w = c[2 + t];
                    s0 += (int)p[3 * t] * w;
                    s1 += (int)p[3 * t + 1] * w;
                    s2 += (int)p[3 * t + 2] * w;
                }
                tmp[r][3 * j] = (uint8_t)clip8(s0);
                tmp[r][3 * j + 1] = (uint8_t)clip8(s1);
                tmp[r][3 * j + 2] = (uint8_t)clip8(s2);
            }
            __syncthreads();
            // vertical pass: thread j accumulates its column of every output row of the band over the staged rows
            if (tid < S) {
#pragma unroll
                for (int ii = 0; ii < BAND; ++ii) {
                    const int32_t* r = vc + (int64_t)(i0 + ii) * (2 + d.kv);
                    const int ymin = min(max(r[0], 0), d.H - 1);
                    const int n = min(min(max(r[1], 0), d.kv), d.H - ymin);
                    const int lo = max(ymin, y0), hi = min(ymin + n, y0 + rows);
                    for (int y = lo; y < hi; ++y) {
                        const int w = r[2 + (y - ymin)];
                        const uint8_t* q = &tmp[y - y0][3 * tid];
                        acc[ii][0] += (int)q[0] * w;
                        acc[ii][1] += (int)q[1] * w;
                        acc[ii][2] += (int)q[2] * w;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid >= S) return;
    // ToTensor + Normalize in f32, one rounding per operation: (v / 255 - mean_c) / std_c (torchvision's order; the constants are
    // the double literals rounded to f32, as torch.as_tensor makes them)
    const float mean[3] = {(float)0.48145466, (float)0.4578275, (float)0.40821073};
    const float stdv[3] = {(float)0.26862954, (float)0.26130258, (float)0.27577711};
    const int j = tid;
#pragma unroll
    for (int ii = 0; ii < BAND; ++ii) {
        const int i = i0 + ii;
        const int64_t prow = f * 49 + (i >> 5) * 7 + (j >> 5);
        const int64_t pcol = (int64_t)(i & 31) * 32 + (j & 31);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int u = ok ? clip8(acc[ii][c]) : 0;
            const float v = ok ? __fdiv_rn(__fsub_rn(__fdiv_rn((float)u, 255.f), mean[c]), stdv[c]) : __builtin_nanf("");
            const int64_t e = prow * ldp + c * 1024 + pcol;
            if (dtype == MADE_F32) ((float*)patches)[e] = v;
            else ((bf16_t*)patches)[e] = (bf16_t)v;
            if (crop) crop[((f * S + i) * S + j) * 3 + c] = (uint8_t)u;
        }
    }
}

}  // namespace

extern "C" int made_frames_preprocess(const uint8_t* frames, int64_t frames_bytes, const MadeFrameDesc* desc, int64_t n_frames,
                                      const int32_t* coef, int64_t n_coef, void* patches, int32_t patch_dtype, int64_t ld_patch,
                                      uint8_t* crop_out, void* stream) {
    MADE_REQUIRE(frames && desc && coef && patches, "made_frames_preprocess: null pointer");
    MADE_REQUIRE(n_frames >= 0 && n_frames <= MADE_FRAMES_MAX, "made_frames_preprocess: n_frames must lie in [0, %d]", MADE_FRAMES_MAX);
    MADE_REQUIRE(frames_bytes > 0 && n_coef > 0, "made_frames_preprocess: empty frame buffer or coefficient table");
    MADE_REQUIRE(patch_dtype == MADE_F32 || patch_dtype == MADE_BF16, "made_frames_preprocess: patch_dtype must be MADE_F32 or MADE_BF16");
    MADE_REQUIRE(ld_patch >= 3 * 32 * 32, "made_frames_preprocess: ld_patch must be >= 3072");
    if (n_frames == 0) return MADE_OK;
    hipLaunchKernelGGL(frames_preprocess_kernel, dim3((unsigned)(n_frames * (S / BAND))), dim3(PT), 0, (hipStream_t)stream, frames,
                       frames_bytes, desc, coef, n_coef, patches, (int)patch_dtype, ld_patch, crop_out);
    return made_check_launch("made_frames_preprocess");
}
