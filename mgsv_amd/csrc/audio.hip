// Audio for the AST tower (mgsv_amd/music.py): decoded PCM -> 16 kHz -> Kaldi fbank segments -> the patch rows of AST's patch
// embedding.  Restates what the reference computes from raw audio (dataloaders/dataloader_MGSV_EC_rawdata.py:95-158): torchaudio's
// resample (made_audio_resample), kaldi.fbank + AST's padding and normalisation (made_audio_fbank), and the im2col of AST's 16 x 16,
// stride 10 Conv2d over the transposed spectrogram (made_ast_patches).  Every table (taps, window, twiddles, mel filters) is computed
// on the host in float64 and rounded to f32; the kernels do f32 arithmetic only.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------- resample
constexpr int RT = 256;                                // threads
constexpr int RPT = MADE_RESAMPLE_TILE / RT;           // outputs per thread
constexpr int SLAB = MADE_RESAMPLE_SLAB;
static_assert(MADE_RESAMPLE_TILE % RT == 0, "tile split");

// workgroup x: track x / tiles, outputs (x % tiles) * TILE ...  Thread tid owns outputs j0 + r * RT + tid, so the lanes of a wave
// hold consecutive phases p (coalesced reads of the k-major taps) and (nearly) the same input block b (LDS broadcast).
__global__ __launch_bounds__(RT) void resample_kernel(const float* __restrict__ pcm, int64_t pcm_len, const MadeResampleDesc* __restrict__ desc,
                                                     const float* __restrict__ taps, int64_t n_taps, float* __restrict__ out, int64_t out_len,
                                                     int64_t tiles) {
    __shared__ float slab[SLAB];
    const int64_t t = blockIdx.x / tiles;
    const int64_t j0 = (int64_t)(blockIdx.x % tiles) * MADE_RESAMPLE_TILE;
    const int tid = threadIdx.x;
    const MadeResampleDesc d = desc[t];
    float* y = out + t * out_len;
    const int64_t jend = min(j0 + (int64_t)MADE_RESAMPLE_TILE, out_len);
    const bool copy = d.o == 1 && d.m == 1;
    const int64_t ntap = 2 * (int64_t)d.width + d.o;
    bool ok = d.o >= 1 && d.m >= 1 && d.width >= 0 && d.n >= 0 && d.offset >= 0 && d.offset + d.n <= pcm_len;
    if (ok && !copy)
        ok = d.taps >= 0 && d.taps + ntap * d.m <= n_taps && ((MADE_RESAMPLE_TILE - 1) / d.m + 1) * (int64_t)d.o + ntap <= SLAB;
    if (!ok) {
        for (int64_t j = j0 + tid; j < jend; j += RT) y[j] = __builtin_nanf("");
        return;
    }
    const float* x = pcm + d.offset;
    if (copy) {
        for (int64_t j = j0 + tid; j < jend; j += RT) y[j] = j < d.n ? x[j] : 0.f;
        return;
    }
    const int64_t n_out = (d.m * d.n + d.o - 1) / d.o;            // ceil(m n / o): torchaudio's target length
    const int64_t nval = min(jend, n_out);
    const int64_t b_first = j0 / d.m;
    if (j0 < nval) {
        // x~[b_first o .. b_last o + ntap) = x[b_first o - width ..], zero outside the track
        const int64_t s0 = b_first * d.o - d.width;
        const int len = (int)(((nval - 1) / d.m - b_first) * d.o + ntap);
        for (int i = tid; i < len; i += RT) {
            const int64_t xi = s0 + i;
            slab[i] = (xi >= 0 && xi < d.n) ? x[xi] : 0.f;
        }
    }
    __syncthreads();
    if (j0 >= nval) {
        for (int64_t j = j0 + tid; j < jend; j += RT) y[j] = 0.f;
        return;
    }
    // the RPT outputs of a thread share the k loop: RPT independent tap loads and FMA chains in flight (an output past nval reads
    // output j0's operands and is not stored)
    const float* K = taps + d.taps;
    const float* xs[RPT];
    const float* kp[RPT];
    float acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t j = j0 + r * RT + tid;
        const int64_t jc = j < nval ? j : j0;
        const int64_t b = jc / d.m;
        xs[r] = slab + (b - b_first) * d.o;
        kp[r] = K + (jc - b * d.m);
        acc[r] = 0.f;
    }
    for (int k = 0; k < (int)ntap; ++k) {
        const int64_t ko = (int64_t)k * d.m;
#pragma unroll
        for (int r = 0; r < RPT; ++r) acc[r] = fmaf(kp[r][ko], xs[r][k], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int64_t j = j0 + r * RT + tid;
        if (j < jend) y[j] = j < nval ? acc[r] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- fbank
constexpr int FT = 256;                 // threads: 4 waves, one frame each per pass
constexpr int FW = FT / WAVE;           // frames per pass
constexpr int FROWS = 16;               // spectrogram rows per workgroup
constexpr int NFFT = 512, WIN = 400, SHIFT = 160;
constexpr int NROW = MADE_AUDIO_ROWS, NMEL = MADE_AUDIO_MELS;
static_assert(NROW % FROWS == 0 && FROWS % FW == 0, "row tiles");
constexpr float NORM_MEAN = 4.2677393f, NORM_DIV = 9.1379948f;   // (x - (-4.2677393)) / (4.5689974 * 2), in f32
constexpr float LOG_FLOOR_ARG = 1.1920928955078125e-07f;          // torch.finfo(float32).eps
constexpr float LOG_FLOOR = -15.942384719848633f;                 // log(2^-23) rounded to f32

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = WAVE / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// workgroup x: segment x / (NROW / FROWS), rows (x % (NROW / FROWS)) * FROWS ...; pass q of the row loop gives wave w row r0 + 4 q + w
__global__ __launch_bounds__(FT) void fbank_kernel(const float* __restrict__ pcm, int64_t pcm_len, const MadeAudioSegDesc* __restrict__ segs,
                                                   const float* __restrict__ window, const float* __restrict__ twiddle,
                                                   const float* __restrict__ mel, int mel_ld, float* __restrict__ spec) {
    __shared__ float re[FW][NFFT], im[FW][NFFT];
    __shared__ float tw[NFFT];
    const int64_t s = blockIdx.x / (NROW / FROWS);
    const int r0 = (int)(blockIdx.x % (NROW / FROWS)) * FROWS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & (WAVE - 1);
    const MadeAudioSegDesc d = segs[s];
    const bool ok = d.first >= 0 && d.count >= 0 && d.first + d.count <= pcm_len;
    const int nf = !ok ? 0 : (d.count < WIN ? 0 : (int)min((int64_t)NROW, 1 + (d.count - WIN) / SHIFT));
    float* rows = spec + (s * NROW + r0) * NMEL;
    const float pad = ok ? __fdiv_rn(NORM_MEAN, NORM_DIV) : __builtin_nanf("");
    for (int i = tid; i < FROWS * NMEL; i += FT)
        if (r0 + i / NMEL >= nf) rows[i] = pad;
    const int hi = min(r0 + FROWS, nf);
    if (r0 >= hi) return;                                          // uniform: the whole tile is padding
    for (int i = tid; i < NFFT; i += FT) tw[i] = twiddle[i];
    float* fre = re[wave];
    float* fim = im[wave];
    for (int rb = r0; rb < hi; rb += FW) {
        const int r = rb + wave;
        const bool act = r < hi;
        if (act) {
            // mean removal, pre-emphasis (y[0] = x[0] - 0.97 x[0]), the window; written bit-reversed, zero-padded to 512
            const float* x = pcm + d.first + (int64_t)r * SHIFT;
            float sum = 0.f;
            for (int i = lane; i < WIN; i += WAVE) sum += x[i];
            const float mean = __fdiv_rn(wave_sum(sum), (float)WIN);
            for (int i = lane; i < NFFT; i += WAVE) {
                float v = 0.f;
                if (i < WIN) {
                    const float a = __fsub_rn(x[i], mean);
                    const float b = __fsub_rn(x[i > 0 ? i - 1 : 0], mean);
                    v = __fmul_rn(__fsub_rn(a, __fmul_rn(0.97f, b)), window[i]);
                }
                const int br = (int)(__brev((unsigned)i) >> 23);
                fre[br] = v;
                fim[br] = 0.f;
            }
        }
        __syncthreads();
        // radix-2 decimation in time: stage st joins blocks of 2^st; twiddle exp(-2 pi i pos / 2^(st+1)) = tw[pos << (8 - st)]
        for (int st = 0; st < 9; ++st) {
            if (act) {
                const int half = 1 << st;
#pragma unroll
                for (int q = lane; q < NFFT / 2; q += WAVE) {
                    const int pos = q & (half - 1);
                    const int a = ((q >> st) << (st + 1)) + pos, b = a + half;
                    const int k = pos << (8 - st);
                    const float c = tw[k], sn = tw[NFFT / 2 + k];
                    const float br_ = fre[b], bi = fim[b];
                    const float tr = fmaf(c, br_, sn * bi), ti = fmaf(c, bi, -sn * br_);
                    const float ar = fre[a], ai = fim[a];
                    fre[a] = ar + tr;
                    fim[a] = ai + ti;
                    fre[b] = ar - tr;
                    fim[b] = ai - ti;
                }
            }
            __syncthreads();
        }
        if (act) {
            // |X_j|^2 for j < 256 (the Nyquist bin has weight 0 in every filter); each lane rewrites only the bins it read
#pragma unroll
            for (int j = lane; j < NFFT / 2; j += WAVE) fim[j] = fmaf(fre[j], fre[j], fim[j] * fim[j]);
        }
        __syncthreads();
        if (act) {
            float* o = rows + (int64_t)(r - r0) * NMEL;
            for (int bn = lane; bn < NMEL; bn += WAVE) {
                const float* f = mel + (int64_t)bn * mel_ld;
                const int first = min(max((int)f[0], 0), NFFT / 2), cnt = min(max((int)f[1], 0), min(mel_ld - 2, NFFT / 2 - first));
                float e = 0.f;
                for (int t = 0; t < cnt; ++t) e = fmaf(f[2 + t], fim[first + t], e);
                const float lg = e <= LOG_FLOOR_ARG ? LOG_FLOOR : logf(e);        // max(e, eps).log(); NaN stays NaN
                o[bn] = __fdiv_rn(__fadd_rn(lg, NORM_MEAN), NORM_DIV);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- patches
constexpr int PT = 256;
constexpr int NP_F = 12, NP_T = 101, NPATCH = NP_F * NP_T;

__global__ __launch_bounds__(PT) void ast_patches_kernel(const float* __restrict__ spec, int64_t total, void* patches, int dtype, int64_t ldp) {
    for (int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x; e < total; e += (int64_t)gridDim.x * PT) {
        const int64_t row = e >> 8;
        const int c = (int)(e & 255);
        const int64_t s = row / NPATCH;
        const int p = (int)(row - s * NPATCH);
        const int fi = p / NP_T, ti = p - fi * NP_T;
        const int k = c >> 4, l = c & 15;
        const float v = spec[(s * NROW + 10 * ti + l) * NMEL + 10 * fi + k];
        const int64_t o = row * ldp + c;
        if (dtype == MADE_F32) ((float*)patches)[o] = v;
        else ((bf16_t*)patches)[o] = (bf16_t)v;
    }
}

}  // namespace

extern "C" int made_audio_resample(const float* pcm, int64_t pcm_len, const MadeResampleDesc* desc, int64_t n_tracks, const float* taps,
                                   int64_t n_taps, float* out, int64_t out_len, void* stream) {
    MADE_REQUIRE(pcm && desc && taps && out, "made_audio_resample: null pointer");
    MADE_REQUIRE(n_tracks >= 0 && n_tracks <= MADE_AUDIO_TRACKS_MAX, "made_audio_resample: n_tracks must lie in [0, %d]", MADE_AUDIO_TRACKS_MAX);
    MADE_REQUIRE(pcm_len > 0 && n_taps > 0, "made_audio_resample: empty sample buffer or tap table");
    MADE_REQUIRE(out_len >= 0 && out_len <= ((int64_t)1 << 31), "made_audio_resample: out_len must lie in [0, 2^31]");
    if (n_tracks == 0 || out_len == 0) return MADE_OK;
    const int64_t tiles = (out_len + MADE_RESAMPLE_TILE - 1) / MADE_RESAMPLE_TILE;
    MADE_REQUIRE(n_tracks * tiles < ((int64_t)1 << 31), "made_audio_resample: n_tracks * out_len too large for one launch");
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(n_tracks * tiles)), dim3(RT), 0, (hipStream_t)stream, pcm, pcm_len, desc, taps,
                       n_taps, out, out_len, tiles);
    return made_check_launch("made_audio_resample");
}

extern "C" int made_audio_fbank(const float* pcm, int64_t pcm_len, const MadeAudioSegDesc* segs, int64_t n_segs, const float* window,
                                const float* twiddle, const float* mel, int32_t mel_ld, float* spec, void* stream) {
    MADE_REQUIRE(pcm && segs && window && twiddle && mel && spec, "made_audio_fbank: null pointer");
    MADE_REQUIRE(n_segs >= 0 && n_segs <= MADE_AUDIO_SEGS_MAX, "made_audio_fbank: n_segs must lie in [0, %d]", MADE_AUDIO_SEGS_MAX);
    MADE_REQUIRE(pcm_len > 0, "made_audio_fbank: empty sample buffer");
    MADE_REQUIRE(mel_ld >= 3, "made_audio_fbank: mel_ld must be >= 3");
    if (n_segs == 0) return MADE_OK;
    hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)(n_segs * (NROW / FROWS))), dim3(FT), 0, (hipStream_t)stream, pcm, pcm_len, segs, window,
                       twiddle, mel, (int)mel_ld, spec);
    return made_check_launch("made_audio_fbank");
}

extern "C" int made_ast_patches(const float* spec, int64_t n_segs, void* patches, int32_t patch_dtype, int64_t ld_patch, void* stream) {
    MADE_REQUIRE(spec && patches, "made_ast_patches: null pointer");
    MADE_REQUIRE(n_segs >= 0 && n_segs <= MADE_AUDIO_SEGS_MAX, "made_ast_patches: n_segs must lie in [0, %d]", MADE_AUDIO_SEGS_MAX);
    MADE_REQUIRE(patch_dtype == MADE_F32 || patch_dtype == MADE_BF16, "made_ast_patches: patch_dtype must be MADE_F32 or MADE_BF16");
    MADE_REQUIRE(ld_patch >= 256, "made_ast_patches: ld_patch must be >= 256");
    if (n_segs == 0) return MADE_OK;
    const int64_t total = n_segs * NPATCH * 256;
    const int64_t blocks = min((total + PT - 1) / PT, (int64_t)1 << 20);
    hipLaunchKernelGGL(ast_patches_kernel, dim3((unsigned)blocks), dim3(PT), 0, (hipStream_t)stream, spec, total, patches, (int)patch_dtype, ld_patch);
    return made_check_launch("made_ast_patches");
}
