/*
 * made_hip.h -- C ABI of libmade_hip.so: the MI355X (gfx950) kernels behind the MaDe hot path.
 *
 * The reference (xxayt/MGSV) has NO native/FFI layer: every op on its hot path is a stock ATen
 * call made from Python (SURVEY.md section 2 "Native components: none").  The drop-in boundary is
 * therefore the Python class `Uni_model` (reference model/model_Uni.py:15,177) and this C ABI is
 * the contract the build defines underneath it ("C-ABI level").  Each entry
 * point cites the reference call sites whose arithmetic it replaces.
 *
 * Conventions
 *   - every argument is POD: device pointers, int64 sizes/strides (in ELEMENTS), dtype enums;
 *   - the caller allocates all outputs and workspaces; the library owns no memory;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and returns without
 *     synchronising; return value 0 = OK, < 0 = error (text via made_last_error(), thread-local);
 *   - nothing throws across the boundary; calls are re-entrant on distinct streams;
 *   - masks are float32 with 1 = valid, 0 = padding, exactly as the reference's dataset emits them
 *     (reference dataloaders/dataloader_MGSV_EC_feature.py:61,67).
 */
#ifndef MADE_HIP_H
#define MADE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MADE_ABI_VERSION 9

enum MadeDtype { MADE_F32 = 0, MADE_BF16 = 1 };

enum MadeAct {
    MADE_ACT_NONE = 0,
    MADE_ACT_RELU = 1,       /* DETR FFN / MLP heads: reference music_detr/transformer.py:205,302,358 */
    MADE_ACT_GELU = 2,       /* erf GELU, temporal block FFN: reference model/model_Base.py:72 */
    MADE_ACT_QUICKGELU = 3,  /* x*sigmoid(1.702x): reference model/model_Base.py:17-20 */
    MADE_ACT_SIGMOID = 4     /* span head: reference model/model_Uni.py:135 */
};

/* act'(.) factors of the backward Linears (made_linear `gate`): out = (A W^T) * act'(G) * gate_scale */
enum MadeGate {
    MADE_GATE_NONE = 0,
    MADE_GATE_RELU_OUT = 1,      /* G = saved output of ReLU (after dropout): 1 where G != 0 */
    MADE_GATE_GELU_Z = 2,        /* G = saved pre-activation of the erf GELU */
    MADE_GATE_QUICKGELU_Z = 3,   /* G = saved pre-activation of x*sigmoid(1.702x) */
    MADE_GATE_SIGMOID_OUT = 4    /* G = saved sigmoid output: G (1 - G) */
};

/* Stateless dropout: keep(seed, site, idx) <=> (made_rng_mix(seed, site, idx) >> 8) >= floor(p * 2^24); kept values are
 * scaled by 1/(1-p).  Forward and backward kernels regenerate the same mask from (seed, site, logical element index), so
 * no mask is ever stored (mgsv_amd/dropout.py documents the index conventions and restates the mix in numpy).
 * Replaces torch's Philox draws at reference model/model_Base.py:69-75, modules/transformer.py:177,
 * music_detr/transformer.py:153-162,229-241 (value semantics identical, stream different by construction). */
typedef struct MadeDropout {
    uint64_t seed;
    uint32_t site;
    float    p;              /* 0 = no dropout */
    const uint64_t* seed_device;   /* non-NULL: the kernels read the seed from this device word instead of `seed`, so a captured
                                      hipGraph of the training step draws fresh masks on every replay (the host updates one word) */
} MadeDropout;

#if defined(__HIPCC__)
#define MADE_HOST_DEVICE __host__ __device__      /* the kernels call the same definition */
#else
#define MADE_HOST_DEVICE
#endif
MADE_HOST_DEVICE static inline uint32_t made_rng_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
/* keep threshold of probability p (a float32): floor(p * 2^24), evaluated exactly */
MADE_HOST_DEVICE static inline uint32_t made_drop_threshold(float p) { return (uint32_t)((double)p * 16777216.0); }
/* mix(seed, site, idx) = fmix32(lo32(idx) ^ key(seed, site, hi32(idx))): kernels hoist the key out of their inner loops */
MADE_HOST_DEVICE static inline uint32_t made_rng_key(uint64_t seed, uint32_t site, uint32_t idx_hi) {
    return made_rng_fmix32((uint32_t)seed ^ (site * 0x9E3779B9u) ^ ((uint32_t)(seed >> 32) * 0x85EBCA6Bu) ^ (idx_hi * 0xC2B2AE35u));
}
MADE_HOST_DEVICE static inline uint32_t made_rng_mix(uint64_t seed, uint32_t site, uint64_t idx) {
    return made_rng_fmix32((uint32_t)idx ^ made_rng_key(seed, site, (uint32_t)(idx >> 32)));
}
#if defined(__HIPCC__)
/* the seed a kernel uses: one scalar load per kernel when it lives in device memory */
__device__ static inline uint64_t made_drop_seed(const MadeDropout& d) { return d.seed_device ? *d.seed_device : d.seed; }
#endif


enum MadeStatus {
    MADE_OK = 0,
    MADE_ERR_INVALID_ARG = -1,
    MADE_ERR_UNSUPPORTED = -2,
    MADE_ERR_HIP = -3
};

int         made_abi_version(void);
/* f32 products (the `f32_products` field of MadeLinearArgs, MadeAttnArgs, MadeWideAttnArgs, MadeAttnBwdArgs and MadeGemmTNArgs): how THAT call
 * multiplies f32 operands (MadeDtype MADE_F32 compute).  0 = exact (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak); 1 = split-bf16: each operand as
 * hi + lo bf16 halves and a . b ~ hi.hi + hi.lo + lo.hi on the bf16 matrix pipe (three products at 16x the f32 rate; the operands' last 7
 * mantissa bits are dropped: relative 8e-6 per operand, f32 accumulation, storage and elementwise steps unchanged); any other value is
 * MADE_ERR_INVALID_ARG.  The field has no effect on a call that multiplies no f32 operands (bf16 compute).  The library keeps no mode of
 * its own: every launch is what its arguments say.  The reference's arithmetic is fp32 throughout (train-MaDe.py:237), its tolerance
 * <= 1e-4 on logits / spans -- the engine's "f32x3" mode is held to that gate by the same tests as "f32". */
const char* made_last_error(void);
/* fills name (<= name_len chars), compute-unit count and 1 if the device is gfx950 */
int         made_device_info(char* name, int name_len, int* cu_count, int* is_gfx950);

/* ------------------------------------------------------------------------------------------
 * made_linear: out = act(A' W^T + bias) (+ R), the fused Linear of the path.
 * Replaces: nn.Linear at reference model/model_Base.py:559,598 (vit_proj/ast_proj, with the
 * masked_fill of :556,:595 as `a_row_mask` and the PE add of :533 as `R` with r_row_mod=T),
 * :75-80,:81 (temporal FFN / final_linear, masked_fill :541 as `out_row_mask`), the packed in-proj
 * and out-proj of every nn.MultiheadAttention (reference music_detr/transformer.py:153,229,230;
 * model/model_Base.py:69) with the `with_pos_embed` adds of :193,:284,:293-294 as `A2`, FFN
 * linears :205,:302, heads at reference model/model_Uni.py:131-146 and the X-Pool projections
 * reference modules/transformer.py:96-103,122,176.
 *
 *   A' = (A + A2[row % a2_row_mod]) for column segments flagged use_a2 (or A2 itself when a2_replace is set),
 *   else A; rows of A whose a_row_mask is 0 are read as zero.  W is [N,K] row-major (nn.Linear layout), K contiguous.
 *   Compute type = w_dtype: MADE_BF16 -> v_mfma_f32_32x32x16_bf16, MADE_F32 -> v_mfma_f32_32x32x2_f32
 *   (exact f32 FMA chain; three bf16 products on split operands when f32_products = 1); accumulation is always f32.
 *   The N columns are split into up to 4 segments, each with its own output tensor; a segment may
 *   be written transposed per batch (out[b][n][t], t = row % rows_per_batch) which is the layout
 *   made_attention wants for V.  `batch` > 1 runs independent problems (grid.z) with the given
 *   element strides (used for the per-track QK^T / PV products of the X-Pool block).
 *   split_k > 1 (skinny problems: the decoder's M = B*Q rows): grid.z splits K, every block writes its raw
 *   f32 partial tile to split_ws[split][M][N] and NO epilogue runs; made_splitk_finish sums the splits and
 *   applies bias / act / residual (and optionally LayerNorm), so a 64-row GEMM fills the chip.
 */
typedef struct MadeLinearSeg {
    int64_t col_begin;         /* first column of this segment (multiple of 128 unless nseg == 1) */
    void*   out;
    int32_t out_dtype;         /* MadeDtype */
    int32_t transposed;        /* 0: out[row*ldo + col]; 1: out[(row/rpb)*obs + col*ldo + row%rpb] */
    int64_t ldo;
    int64_t rows_per_batch;    /* rpb; 0 = plain rows */
    int64_t out_batch_stride;  /* obs (elements), used when rows_per_batch > 0 */
    int64_t out_z_stride;      /* per-problem stride when batch > 1 */
    int32_t use_a2;
    int32_t _pad;
} MadeLinearSeg;

typedef struct MadeLinearArgs {
    const void*  A;  int32_t a_dtype; int32_t w_dtype;
    int64_t      lda;
    const void*  A2; int64_t lda2; int64_t a2_row_mod;      /* A2 has a_dtype; may be NULL */
    int32_t      a2_replace;                                /* 1: flagged segments read A2 INSTEAD of A (e.g. src+pos) */
    int32_t      drop_col_div;                              /* > 1: dropout draws once per `drop_col_div` columns -- element index
                                                               row * drop_ld + col / drop_col_div (one attention-weight draw per head
                                                               on the value path of a one-query self-attention); 0 / 1: per element */
    const float* a_row_mask;                                /* [M] or NULL */
    const void*  W;  int64_t ldw;
    const float* bias;                                      /* [N] f32 or NULL */
    int64_t      M, N, K;
    int64_t      batch, a_z_stride, w_z_stride;             /* batch >= 1 */
    int32_t      act; int32_t r_dtype;
    const void*  R;  int64_t ldr; int64_t r_row_mod;        /* added after act; may be NULL */
    const float* out_row_mask;                              /* [M] or NULL: masked rows -> 0 */
    const float* tile_skip_mask;                            /* [M] or NULL: a tile whose rows are ALL 0 here is not computed
                                                               (its rows are left untouched, or zeroed when out_row_mask is
                                                               set): padded tokens cost nothing.  Rows are independent, so
                                                               valid rows are unaffected. */
    int32_t      nseg; int32_t split_k;                     /* split_k > 1: see below */
    float*       split_ws;                                  /* [split_k, M, N] f32 workspace or NULL */
    MadeLinearSeg seg[4];
    /* training-path epilogue (plain segments only; element order: z = A'W^T + bias [-> Zout], act, gate, dropout, +R, row mask) */
    const void*  G;  int32_t g_dtype; int32_t gate;         /* MadeGate: multiply by act'(G[row*ldg + col]) * gate_scale */
    int64_t      ldg; float gate_scale; int32_t z_dtype;
    void*        Zout; int64_t ldz;                         /* optional: the pre-activation z is also stored (saved for backward) */
    MadeDropout  drop; int64_t drop_ld;                     /* dropout after act/gate, element index row*drop_ld + col */
    /* row gather (padded tokens cost nothing): the kernel works on logical rows r < *n_rows (device scalar) that live at
       physical rows row_index[r] of A / A2 / R / G / out / masks (made_row_index of the token mask); every per-row quantity
       (residual, dropout index, rows_per_batch addressing) keeps using the PHYSICAL row, so valid rows are bit-identical to
       the ungathered call and padded rows are simply never read or written.  M stays the physical row count. */
    const int32_t* row_index; const int32_t* n_rows;
    /* per-(row, problem) scaled bias (tiny-M kernel only): the bias term is bias[z * bias_z_stride + col] * bias_row_scale[row * batch + z]
       for problem z of a batched call -- the value-projection bias of the memory-space cross-attention, whose dropped attention
       weights no longer sum to 1 (reference music_detr/transformer.py:293-296 under dropout; replaces a made_head_bias launch) */
    const float* bias_row_scale; int64_t bias_z_stride;
    int32_t      f32_products; int32_t _pad;                /* 0 = exact f32 products, 1 = split-bf16 (see "f32 products" above) */
} MadeLinearArgs;

int made_linear(const MadeLinearArgs* args, void* stream);

/* Which kernel made_linear dispatches these arguments to (no launch; for profilers and bench.py's per-kernel roofline, so a
 * HIP-event average can be set beside rocprofv3's per-symbol average). */
enum MadeLinearVariant {
    MADE_LINEAR_GENERAL_F32 = 0,    /* linear_kernel<float, float>: exact-f32 MFMA, every option */
    MADE_LINEAR_GENERAL_F32IN = 1,  /* linear_kernel<float, bf16>: f32 activations converted in the prologue */
    MADE_LINEAR_GENERAL_BF16 = 2,   /* linear_kernel<bf16, bf16>: split-K, additive A2, transposed segments */
    MADE_LINEAR_TINY = 3,           /* linear_tiny_kernel: 64 x 32 tiles, fragments straight from global memory (K <= 1024) */
    MADE_LINEAR_SKINNY = 4,         /* linear_skinny_kernel: 64 x 64 tiles, 8-stage LDS-DMA ring */
    MADE_LINEAR_GLDS3 = 5,          /* linear_glds_kernel<3, ., 128>: at most one workgroup per CU, three LDS stages */
    MADE_LINEAR_GLDS64 = 6,         /* linear_glds_kernel<1, ., 64>: 64 x 128 tiles */
    MADE_LINEAR_GLDS128 = 7,        /* linear_glds_kernel<1, ., 128>: 128 x 128 tiles */
    MADE_LINEAR_BIG256 = 8,         /* linear_big_kernel<256>: persistent, 256 x 256 tiles, two LDS stages, register epilogue (round 4; the
                                       slot was round 2's ring kernel, removed) */
    MADE_LINEAR_TINY16 = 9,         /* linear_t16_kernel: at most 64 rows, 16 x 16 tiles (a third of the bytes per workgroup), 128 <= K <= 1024 */
    MADE_LINEAR_BIG128 = 10,        /* linear_big_kernel<128>: the same with 128 x 256 tiles (MADE_LINEAR_TILE=256; the slot was round 3's
                                       W-stationary kernel, removed) */
    MADE_LINEAR_GLDS64_F32 = 11,    /* linear_glds_kernel<1, ., 64, float>: the f32 parity mode's large Linears on the LDS-DMA loop (exact-f32 MFMA) */
    MADE_LINEAR_GLDS128_F32 = 12    /* linear_glds_kernel<1, ., 128, float> */
};
int made_linear_variant(const MadeLinearArgs* args);

/* One stage of the moment-DETR decoder's chain of B*Q-row Linears with the PREVIOUS stage's LayerNorm in its prologue
 * (reference music_detr/transformer.py:273-307, forward_post; :136 for the shared output norm):
 *     x   = LayerNorm(Zin; ln_g, ln_b)          Zin raw rows [M, K] (f32, or bf16 in the training chain); ln_g == NULL: x = Zin
 *     x2  = LayerNorm(x; ln2_g, ln2_b)          optional -> x2_out (bf16): the decoder output of the previous layer
 *     A   = bf16(x) (+ add[row % add_row_mod])  add: bf16 rows of K elements (query_pos) or NULL; x itself -> x_out (bf16) or NULL
 *     out = act(A W^T + bias) + R               R: bf16 [M, N] or NULL; res_from_x: + bf16(x) instead (needs N == K, no add)
 * bf16 MFMA, f32 accumulate; K (the LayerNorm width) is 256 or 512; out is f32 (raw rows for the next stage's norm) or bf16.
 * One launch of ceil(N / 16) x ceil(M / 16) workgroups (16 x 16 tiles), no split-K workspace, no finish launch.
 * Where the kernels round (everything else is f32):
 *   - the f32-row instances take mean and variance in two passes (centred); the bf16-row instances take them in ONE pass,
 *     var = max(Sxx / K - mean^2, 0).  The second norm is two-pass in every instance and reads the f32 x, not the stored one.
 *   - x_out = bf16(x), x2_out = bf16(x2).
 *   - A = bf16(x) without add; with add, A = bf16(bf16(x) + add), the sum taken in f32.  a_out holds the same bits as the matrix operand.
 *   - the product takes the bf16 A and W and accumulates in f32; bias, activation, dropout (x 1 / (1 - p), dropped: +0) and the
 *     residual follow in f32; res_from_x adds bf16(x); out is rounded once at the store (bf16) or not at all (f32).
 *   - dropout draws element row * drop_ld + col / max(drop_col_div, 1) whatever ldo is.
 * Rows M .. of the last row tile and columns N .. of the last column tile are computed on clamped addresses and never stored. */
typedef struct MadeDecStageArgs {
    const void*  Zin; int64_t ldz;                 /* f32 rows (zin_dtype = MADE_F32, the eval chain) or bf16 rows (MADE_BF16, the training chain) */
    const float* ln_g; const float* ln_b;
    const float* ln2_g; const float* ln2_b; void* x2_out; int64_t ldx2;
    const void*  add; int64_t add_row_mod;
    void*        x_out; int64_t ldx;
    const void*  W; int64_t ldw; const float* bias;
    const void*  R; int64_t ldr;
    void*        out; int64_t ldo;
    int32_t      out_dtype; int32_t act; int32_t res_from_x; float eps;
    int64_t      M, N, K;
    /* training chain (bf16 Zin only): A = bf16(x) + add is also stored (a_out: the weight gradient's operand), and the stateless
       dropout of this header follows the activation -- element index row * drop_ld + col / max(drop_col_div, 1) */
    int32_t      zin_dtype; int32_t drop_col_div;
    void*        a_out; int64_t lda_out;
    MadeDropout  drop; int64_t drop_ld;
} MadeDecStageArgs;
int made_dec_stage(const MadeDecStageArgs* args, void* stream);

/* Which kernel instance made_dec_stage runs these arguments on, or the negative status with which it refuses them (every argument
 * check of made_dec_stage lives here; no launch). */
enum MadeDecStageVariant {
    MADE_DEC_STAGE_256_F32 = 0,     /* dec_stage_kernel<4, false, false>: K = 256, f32 rows (the eval chain) */
    MADE_DEC_STAGE_256_BF16 = 1,    /* dec_stage_kernel<4, true, true>: K = 256, bf16 rows, the training options */
    MADE_DEC_STAGE_512_F32 = 2,     /* dec_stage_kernel<8, false, false> */
    MADE_DEC_STAGE_512_BF16 = 3     /* dec_stage_kernel<8, true, true> */
};
int made_dec_stage_variant(const MadeDecStageArgs* args);

/* made_dec_stage_bwd: a stage of the decoder's BACKWARD chain with a LayerNorm backward in the prologue of the dX product that
 * consumes it (reference music_detr/transformer.py:273-307 read backwards; bf16 rows, K = the norm's width = 256 or 512):
 *     g   = dy (+ add),  or with a second norm stacked on the first (xb != NULL: norm 3 + the shared output norm, :306 and :136)
 *     g   = LN_b'(dy; xb, gamma_b) + add
 *     dx  = LN_a'(g; xa, gamma_a)       -> dx_out [M, K] (may be NULL);  dgamma / dbeta of the norm(s) accumulated (may be NULL)
 *     A   = dropout_a(dx)               -> a_out [M, K] (may be NULL): element index row * drop_a_ld + col
 *     out = dropout_o((A W^T) * [G != 0] * gate_scale) + R        W [N, K] bf16; G, R, out [M, N] bf16; drop_o index row * drop_o_ld + col / drop_o_col_div
 * One launch of ceil(N / 16) x ceil(M / 16) workgroups (16 x 16 tiles) replaces made_layernorm_bwd (or made_layernorm_bwd2) + made_linear.
 * Where the kernels round (everything else is f32):
 *   - every LayerNorm backward takes all four row sums (Sx, Sxx, Sg, Sgx; g = dy * gamma) in ONE pass:
 *     mean = Sx / K, var = max(Sxx / K - mean^2, 0), s1 = Sg / K, s2 = rstd (Sgx - mean Sg) / K, dx = rstd (g - s1 - xhat s2).
 *   - dy + add (one norm) and the inner g = LN_b'(dy) + add (two norms) stay in f32.
 *   - dx_out = bf16(dx);  A = bf16(dropout_a(dx)) (x 1 / (1 - p), dropped: +0), rounded separately from dx_out; a_out holds the bits
 *     of the matrix operand.
 *   - the product takes the bf16 A and W and accumulates in f32; gate (G == +-0: +0), gate_scale, dropout_o and R follow in f32; out is
 *     rounded once at the store.
 *   - dgamma / dbeta: dgamma += sum_rows dy * xhat, dbeta += sum_rows dy (for norm a with dy = g).  The workgroups of column tile 0 alone
 *     accumulate them, with ONE f32 atomic per column and row tile of 16 rows; the pad rows of a ragged last tile add nothing.  With
 *     M <= 16 the result is therefore reproducible bit for bit, beyond that up to the order of ceil(M / 16) atomics per column. */
typedef struct MadeDecStageBwdArgs {
    const void* xa; const float* gamma_a; int64_t ldxa;
    const void* xb; const float* gamma_b; int64_t ldxb;      /* second (outer) norm or NULL */
    const void* dy; int64_t lddy;
    const void* add; int64_t ldadd;                          /* may be NULL */
    void* dx_out; int64_t lddx;
    void* a_out; int64_t lda_out;
    float *dgamma_a, *dbeta_a, *dgamma_b, *dbeta_b;
    MadeDropout drop_a; int64_t drop_a_ld;
    const void* W; int64_t ldw;
    const void* G; int64_t ldg; float gate_scale; float eps;
    MadeDropout drop_o; int64_t drop_o_ld; int32_t drop_o_col_div; int32_t _pad;
    const void* R; int64_t ldr;
    void* out; int64_t ldo;
    int64_t M, N, K;
} MadeDecStageBwdArgs;
int made_dec_stage_bwd(const MadeDecStageBwdArgs* args, void* stream);

/* The same for made_dec_stage_bwd: the instance code, or the negative status (no launch). */
enum MadeDecStageBwdVariant {
    MADE_DEC_STAGE_BWD_256_ONE = 0, /* dec_stage_bwd_kernel<4, 0>: K = 256, one norm */
    MADE_DEC_STAGE_BWD_256_ADD = 1, /* dec_stage_bwd_kernel<4, 1>: one norm, g = dy + add */
    MADE_DEC_STAGE_BWD_256_TWO = 2, /* dec_stage_bwd_kernel<4, 2>: two stacked norms (xb), with or without add */
    MADE_DEC_STAGE_BWD_512_ONE = 3, /* dec_stage_bwd_kernel<8, 0> */
    MADE_DEC_STAGE_BWD_512_ADD = 4, /* dec_stage_bwd_kernel<8, 1> */
    MADE_DEC_STAGE_BWD_512_TWO = 5  /* dec_stage_bwd_kernel<8, 2> */
};
int made_dec_stage_bwd_variant(const MadeDecStageBwdArgs* args);

/* y = act(sum_s ws[s] + bias) + R[row % r_row_mod]  -> out (any dtype, may be NULL);
 * then optionally z1 = LayerNorm(y; ln1) -> ln1_out, and z2 = LayerNorm(z1; ln2) -> ln2_out (the decoder's
 * per-layer norm followed by the shared output norm, reference music_detr/transformer.py:306,136).
 * One wave per row; the LayerNorm variants need N <= 2048.  ws is [split_k, M, N] f32. */
typedef struct MadeFinishArgs {
    const float* ws; int64_t split_k, M, N;
    const float* bias; int32_t act; int32_t r_dtype;
    const void*  R; int64_t ldr; int64_t r_row_mod;
    void* out; int32_t out_dtype; int32_t _pad0; int64_t ldo;
    const float* ln1_g; const float* ln1_b; void* ln1_out; int32_t ln1_dtype; int32_t _pad1; int64_t ln1_ld;
    const float* ln2_g; const float* ln2_b; void* ln2_out; int32_t ln2_dtype; int32_t _pad2; int64_t ln2_ld;
    float eps; int32_t _pad3;
} MadeFinishArgs;

int made_splitk_finish(const MadeFinishArgs* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * made_attention: fused multi-head attention core, softmax(Q K^T * scale + key mask) V, flash
 * style (scores never touch HBM).  Replaces the inner part of nn.MultiheadAttention at reference
 * model/model_Base.py:87 and music_detr/transformer.py:199,287,293-296
 * and the CrossAttention core at reference model/model_Base.py:144-163.
 *   Q  [B, Lq, H*hd]  element (b,i,h,d) at Q + b*q_bs + i*ldq + h*hd + d
 *   K  [B, Lk, H*hd]  likewise with k_bs/ldk
 *   V  [B, Lk, H*hd]  likewise with v_bs/ldv (row-major; transposed on the fly by ds_read_b64_tr_b16)
 *   key_mask [B, Lk] f32, 0 = padded key (-inf before the softmax), may be NULL
 *   q_mask   [B, Lq] f32, 0 = output row forced to 0 AFTER the softmax (reference
 *            model/model_Base.py:163), may be NULL
 *   O  [B, Lq, H*hd] (dtype = compute dtype), element stride ldo / o_bs
 * hd in {32, 64, 128}.  A query whose keys are all masked yields NaN like the reference.
 */
typedef struct MadeAttnArgs {
    const void* Q; const void* K; const void* V; void* O;
    int32_t dtype; int32_t hd;
    int64_t B, H, Lq, Lk;
    int64_t q_bs, ldq, k_bs, ldk, v_bs, ldv, o_bs, ldo;
    const float* key_mask; const float* q_mask;
    float scale; int32_t f32_products;   /* 0 = exact f32 products, 1 = split-bf16 (see "f32 products" above) */
    const float* q_skip_mask;  /* [B, Lq] or NULL: queries that are 0 here are padding whose output nobody reads; 32-query
                                  groups (and whole workgroups) made only of them are skipped and their O rows left untouched */
    /* training path */
    float*      lse;           /* [B, H, Lq] f32 or NULL: log-sum-exp of the scaled, masked scores (+inf for a row with no valid
                                  key), saved for made_attention_bwd */
    MadeDropout drop;          /* dropout on the attention weights (after the softmax, as nn.MultiheadAttention does),
                                  element index ((b*H + h)*Lq + i)*Lk + j */
    const int32_t* batch_order; /* [B] or NULL: a permutation of the batch (made_batch_order: longest sequence first).  Only the
                                  ORDER in which workgroups are issued changes -- a padded batch then finishes with its short
                                  samples instead of waiting on a long one that started last; results are unchanged */
    uint32_t* keep_bits;       /* NULL, or (with drop.p > 0) [B*H*ceil(Lk/32), ld_bits] words: the dropout decisions of this call, for
                                  made_attention_bwd (which then tests a bit per score instead of re-drawing it: the draw is ~11 VALU
                                  instructions).  Row (b*H + h)*ceil(Lk/32) + kt holds, for key tile kt (keys 32 kt .. 32 kt + 31), one word
                                  per query: bit j of the word at slot 32 (i / 32) + s(i % 32) = element (i, 32 kt + j) is KEPT, with
                                  s(q) = 2 ((q & 3) + 4 (q >> 3)) + ((q >> 2) & 1) -- the 32 words of a (key tile, query group) pair are
                                  then the sixteen 64-lane masks of a 32 x 32 MFMA accumulator tile (register e: rows (e & 3) + 8 (e >> 2)
                                  and + 4), which the single-pass backward loads with scalar loads.  ld_bits = a multiple of 32 >= Lq;
                                  words of keys behind the sample's last valid key are not written (and not read) */
    int64_t ld_bits;
} MadeAttnArgs;

int made_attention(const MadeAttnArgs* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * made_attention_wide: single-head attention with head dimension = model width D (256 or 512),
 * keys and values ROW-major, flash style.  O[b, nq, :] = softmax_t(<Q[b,nq], K[b,t]+Kadd[b,t]>*scale
 * + key mask) . V[b, t, :].
 * Replaces (a) the X-Pool attention core, reference modules/transformer.py:110-119 (queries = all
 * videos, shared by every track: q_bs = 0), and (b) the DETR decoder cross-attention of reference
 * music_detr/transformer.py:293-296 evaluated in memory space: with W_k moved onto the query and
 * W_v onto the pooled rows, keys = memory + pos (Kadd), values = memory, and the H*Q rows
 * q'_{h,q} = W_k,h^T q_h are the "queries" -- this removes the [B*L, D] x [D, 2*dec*D] projection of
 * the memory (25 % of the forward flops) for the small Q the model uses.
 *   query index nq = i1*NQ2 + i2 addresses Q at b*q_bs + i1*q_s1 + i2*q_s2 and O at
 *   b*o_bs + i1*o_s1 + i2*o_s2; K/Kadd/V rows at b*{k,kadd,v}_bs + t*ld{k,kadd,v}.
 *   Kadd may be NULL; V may alias K (then loaded once).  key_mask [B, L] f32 or NULL.
 *   dtype = compute dtype of Q/K/Kadd/V; o_dtype = dtype of O.  All-masked rows give NaN.
 */
typedef struct MadeWideAttnArgs {
    const void* Q; const void* K; const void* Kadd; const void* V; void* O;
    const float* key_mask;
    int32_t dtype; int32_t o_dtype;
    int64_t B, NQ1, NQ2, L, D;
    int64_t q_bs, q_s1, q_s2, k_bs, ldk, kadd_bs, ldkadd, v_bs, ldv, o_bs, o_s1, o_s2;
    float scale; int32_t f32_products;   /* 0 = exact f32 products, 1 = split-bf16 (see "f32 products" above) */
    int64_t n_split;           /* > 1: keys are split over grid.z (few queries, long memory: fills the chip) and */
    float*  part_o;            /*      the slices are merged by a second launch; [B, n_split, NQ, D] f32 */
    float*  part_ml;           /*      [B, n_split, NQ, 4] f32 (running max, sum, sum of the dropped weights, unused) */
    /* training path */
    MadeDropout drop;          /* dropout on the attention weights, element index ((b*NQ1 + i1)*NQ2 + i2)*L + key */
    float*  sum_out;           /* [B, NQ1*NQ2] f32 or NULL: sum of the dropped weights of each row (1 without dropout) */
    float*  lse_out;           /* [B, NQ1*NQ2] f32 or NULL: log-sum-exp of the scaled scores of each row (saved for made_attention_wide_bwd) */
} MadeWideAttnArgs;

int made_attention_wide(const MadeWideAttnArgs* args, void* stream);

/* made_attention_wide_bwd: backward of made_attention_wide for the decoder's memory-space cross-attention (few query rows per sample,
 * bf16), one launch per decoder layer (reference music_detr/transformer.py:293-296 under model.train(); replaces a batched Linear,
 * made_softmax_bwd, a batched made_gemm_tn and made_head_bias_bwd on the backward's critical path):
 *   P_j = exp(scale <Q_q, K_j> - lse_q) on valid keys, Pd = dropout(P) (the forward's mask: index (b*NQ + q)*L + j),
 *   dPd_j = <dO_q, V_j> + extra_q,  dS_j = scale P_j (dropout'(dPd_j) - delta_q),  delta_q = <dO_q, O_q> + extra_q ssum_q,
 *   dQ_q = sum_j dS_j K_j.   Pd and dS ([B, NQ, ld_p] bf16, zero on masked keys and on the pad columns L..ld_p-1) are written for
 *   the memory-gradient products dV = Pd^T dO, dK = dS^T Q that follow as one batched made_gemm_tn over all layers.
 * extra_q = gradient of the sum of row q's dropped weights (the value bias enters the forward as ssum_q b_v): `extra` [B, NQ] f32, or,
 * when `extra` is NULL and `dattc` is given, reduced here as <dattc[b, q*hd .. q*hd+hd), vbias[q*hd ..)> (one head per query row).
 * O = the forward's output rows, lse / ssum = its lse_out / sum_out.  Keys may be split over workgroups (n_split, part_dq
 * [B, n_split, NQ, D] f32); the slices' dQ are summed in slice order by a small second launch.  NQ <= 8, D in {256, 512}. */
typedef struct MadeWideAttnBwdArgs {
    const void *Q, *dO, *O, *K, *V;
    const float* key_mask;                 /* [B, L] or NULL */
    const float *lse, *ssum;               /* [B, NQ]; ssum may be NULL (= 1) */
    const float* extra;                    /* [B, NQ] or NULL */
    const void* dattc; int64_t ld_dattc; const float* vbias; int64_t hd;
    void *Pd, *dS; int64_t p_bs, ld_p;
    void* dQ; int64_t dq_bs, ld_dq;
    int64_t B, NQ, L, D;
    int64_t q_bs, ld_q, do_bs, ld_do, o_bs, ld_o, k_bs, ldk, v_bs, ldv;
    float scale; int32_t _pad;
    int64_t n_split; float* part_dq;
    MadeDropout drop;
} MadeWideAttnBwdArgs;
int made_attention_wide_bwd(const MadeWideAttnBwdArgs* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Slice plan of the decoder's memory-space cross-attention: which key tiles (32 keys) every workgroup of made_attention_wide_planned /
 * made_attention_wide_bwd_planned gets.  made_attention_wide(_bwd) cut every sample into n_split equal slices whatever its length, and
 * a launch lasts as long as its longest workgroup; the plan deals the tiles of a padded batch by length instead:
 *   tiles_b = ceil((last valid key of sample b + 1) / 32)      (0: no valid key)
 *   n_b     = max(1, ceil(tiles_b / c))                        (slices of sample b; a sample without a valid key keeps ONE slice of zero
 *                                                               tiles, so that a workgroup defines its outputs)
 *   c       = the smallest cap >= 1 with sum_b n_b <= n_slots and max_b n_b <= max_slices      (made_wide_slice_cap below)
 * and a sample's tiles are dealt evenly over its n_b slices (tiles_b / n_b each, the first tiles_b % n_b slices one more: none
 * longer than c).  Slots are filled in batch_order (made_batch_order: longest first; NULL: sample order), a sample's slices
 * consecutive.  The plan is made once per step on the device from the key mask (one workgroup, nothing read back) and serves every
 * decoder layer, forward and backward.  Layout, int32 words:
 *   [0..3]                    c, used slots, n_slots, max_slices
 *   [4 + 4 b ..]              per sample: tiles_b, first slot, n_b, first valid key (0 when none)
 *   [4 + 4 B + 16 w ..]       per slot w < n_slots (64 bytes): sample (-1: unused slot), first tile, tile count, slice index within the
 *                             sample, first valid key, n_b, tiles_b, 0, then the valid-key bits of the slot's first 8 tiles (bit j of
 *                             word i = key 32 (first tile + i) + j is attended to) -- a workgroup learns all it needs from one load */
#define MADE_WIDE_PLAN_HEAD 4
#define MADE_WIDE_PLAN_SAMPLE 4
#define MADE_WIDE_PLAN_SLOT 16
#define MADE_WIDE_PLAN_SLOT_BITS 8
MADE_HOST_DEVICE static inline int64_t made_wide_plan_words(int64_t B, int64_t n_slots) {
    return MADE_WIDE_PLAN_HEAD + MADE_WIDE_PLAN_SAMPLE * B + MADE_WIDE_PLAN_SLOT * n_slots;
}
/* slices the batch needs under cap c (tiles[b * stride]: the samples' tile counts), or -1 when a sample would need more than max_slices */
MADE_HOST_DEVICE static inline int32_t made_wide_slice_count(const int32_t* tiles, int32_t stride, int32_t B, int32_t c, int32_t max_slices) {
    int32_t total = 0;
    for (int32_t b = 0; b < B; ++b) {
        const int32_t t = tiles[b * stride];
        const int32_t n = t > c ? (t + c - 1) / c : 1;
        if (n > max_slices) return -1;
        total += n;
    }
    return total;
}
/* the cap: the smallest c >= 1 whose slices fit n_slots workgroups and max_slices partial rows per sample; 0: none (B > n_slots) */
MADE_HOST_DEVICE static inline int32_t made_wide_slice_cap(const int32_t* tiles, int32_t stride, int32_t B, int32_t n_slots, int32_t max_slices) {
    int32_t tmax = 1;
    for (int32_t b = 0; b < B; ++b) tmax = tiles[b * stride] > tmax ? tiles[b * stride] : tmax;
    for (int32_t c = 1; c <= tmax; ++c) {
        const int32_t n = made_wide_slice_count(tiles, stride, B, c, max_slices);
        if (n >= 0 && n <= n_slots) return c;
    }
    return 0;
}
/* slice s (< n) of a sample with `tiles` tiles in n slices: first tile and tile count */
MADE_HOST_DEVICE static inline int32_t made_wide_slice_first(int32_t tiles, int32_t n, int32_t s) {
    return s * (tiles / n) + (s < tiles % n ? s : tiles % n);
}
MADE_HOST_DEVICE static inline int32_t made_wide_slice_len(int32_t tiles, int32_t n, int32_t s) { return tiles / n + (s < tiles % n ? 1 : 0); }

/* made_wide_slice_plan: key_mask [B, L] f32 -> plan (plan_bytes >= 4 * made_wide_plan_words(B, n_slots)).  One workgroup;
 * B <= n_slots <= 1024, max_slices >= 1, L <= 32768.
 * made_attention_wide_planned / _bwd_planned: made_attention_wide / _bwd on n_slots workgroups that follow the plan (made from the
 * same key_mask with the same n_slots); args->n_split is the slice CAPACITY of part_o / part_ml / part_dq (>= the plan's max_slices),
 * partial rows at [(b * capacity + slice) * NQ + q].  The merge launches sum a sample's slices 0 .. n_b - 1 in slice order: results
 * are bitwise reproducible from launch to launch.  bf16, D in {256, 512}, no Kadd, a key mask, one query tile per sample
 * (NQ1 * NQ2 <= 32 forward, NQ <= 8 backward); anything else is MADE_ERR_UNSUPPORTED and the caller keeps the unplanned call. */
int made_wide_slice_plan(const float* key_mask, int64_t B, int64_t L, int32_t n_slots, int32_t max_slices,
                         const int32_t* batch_order, void* plan, int64_t plan_bytes, void* stream);
int made_attention_wide_planned(const MadeWideAttnArgs* args, const void* plan, int32_t n_slots, void* stream);
int made_attention_wide_bwd_planned(const MadeWideAttnBwdArgs* args, const void* plan, int32_t n_slots, void* stream);

/* ------------------------------------------------------------------------------------------
 * Launch tape: record the library's launches of one training (or eval) step once, replay them from one C loop.
 * Between made_tape_begin() and made_tape_end() every kernel launch of the calling thread is executed as usual AND appended to the
 * tape (function, grid, block, LDS bytes, stream, argument bytes); made_stream_wait / made_memset_async / made_copy_async are the
 * stream-to-stream dependency, fill and device-to-device copy that are recorded the same way (use them instead of the framework's
 * own calls inside a recorded region).  made_tape_replay re-issues the sequence to the same streams: everything that changes
 * between replays must therefore live in device memory at fixed addresses (batch buffers, MadeDropout.seed_device,
 * MadeAdamDeviceState).  Replaces what the reference gets from the framework's eager dispatch (train-MaDe.py:337-381: ~5 300 ATen
 * dispatches per step); a replayed launch costs the host the HIP runtime's 2-3 us instead of ~10 us of interpreter + ctypes or
 * ~9 us of hipGraphLaunch's node walk, and the two streams keep their overlap. */
int made_tape_begin(void);
int made_tape_end(uint64_t* handle);
int made_tape_replay(uint64_t handle);
int made_tape_free(uint64_t handle);
/* re-orders the ISSUE order of a finished tape so that all its streams are fed at the same time (per-stream order, event order and
 * hence every result unchanged): `main_weight` operations of the busiest stream for one of each other stream, round-robin */
int made_tape_interleave(uint64_t handle, int32_t main_weight);
int made_tape_count(uint64_t handle, int64_t* kernels, int64_t* waits, int64_t* others);
int made_tape_replay_range(uint64_t handle, int64_t first, int64_t count);   /* operations [first, first + count) only, in the tape's issue order:
                                                                               one phase of a step on its own (measurements) */
int made_tape_op(uint64_t handle, int64_t index, int32_t* kind, uint64_t* function, uint64_t* stream, uint32_t* grid3);
                                                              /* what operation `index` is: kind 0 = kernel launch (function = its host-side
                                                                 address, grid3 = workgroups per axis), other kinds: events, fills, copies.
                                                                 Event operations (kind 1 = record on `stream` + wait, 4 = record on `stream`,
                                                                 5 = `stream` waits) return the event's handle in `function`: a wait refers to
                                                                 the latest record of the same handle in front of it */
int made_stream_wait(void* src_stream, void* dst_stream);            /* dst waits for all work queued on src so far */
/* recording only, executes nothing: a HOST callback at this point of the issue order; a replay calls fn(user) there (non-zero return:
 * the replay stops with an error).  For work the library does not launch itself but that must sit between the step's launches: the
 * data-parallel gradient all-reduces (RCCL calls of the framework, reference train-MaDe.py:238-241,371).  made_tape_interleave moves
 * nothing across a callback. */
typedef int (*MadeTapeCallback)(void* user);
int made_tape_callback(MadeTapeCallback fn, void* user);
int made_tape_event(int32_t op_kind, int32_t slot, void* stream);    /* recording only, executes nothing: 0 = "record event `slot` on
                                                                         stream", 1 = "stream waits for event `slot`" -- mirrors the
                                                                         framework's own Event.record / Stream.wait_event calls */
int made_memset_async(void* dst, int32_t value, int64_t nbytes, void* stream);
int made_copy_async(void* dst, const void* src, int64_t nbytes, void* stream);
/* dst[0 .. n_words) = words[0 .. n_words) (n_words <= 4, 32-bit words, dst 4-byte aligned): the words travel as kernel arguments of a
 * one-wave launch, so the call is stream-ordered and the host buffer may be reused at once -- the per-step scalars of a replayed
 * training step (dropout seed, learning rates, step count; replaces the framework's fill kernels in TrainStepGraph.step). */
int made_store_words(void* dst, const uint32_t* words, int32_t n_words, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row kernels (HBM-bound).                                                                   */

/* y = LayerNorm(x) * gamma + beta, eps inside the sqrt; one wave per row, D <= 2048, D % 4 == 0.
 * Input row r sits at x + (r / rpb) * x_batch_stride + (r % rpb) * ldx when rpb = x_rows_per_batch > 0
 * (a [B,T,D] view of a larger buffer), else at x + r * ldx; output rows are y + r * ldy.
 * (rows are independent, so skipping padded rows leaves every valid row bit-identical.)
 * Replaces nn.LayerNorm at reference model/model_Base.py:83,85; music_detr/transformer.py:202,
 * 209,290,300,306,136; modules/transformer.py:164-165,174,178. */
int made_layernorm(const void* x, int32_t x_dtype, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride,
                   const float* gamma, const float* beta,
                   void* y, int32_t y_dtype, int64_t ldy, int64_t rows, int64_t D, float eps,
                   const float* row_skip /* [rows] f32 or NULL: rows that are 0 here (padding) are not computed */, void* stream);

/* Same, plus a second output y2 = y + add (row r of `add` at add + r*ld_add; y2 has y's dtype and stride ldy2):
 * the DETR layers need both src and src + pos (reference music_detr/transformer.py:193), so the norm that produces
 * src also emits src + pos and the next projection reads it directly. gamma == NULL skips the normalisation
 * (y = x), which turns the kernel into a fused copy/add for the first encoder layer. */
int made_layernorm_add(const void* x, int32_t x_dtype, int64_t ldx, const float* gamma, const float* beta,
                       void* y, int32_t y_dtype, int64_t ldy, const void* add, int32_t add_dtype, int64_t ld_add,
                       void* y2, int64_t ldy2, int64_t rows, int64_t D, float eps, const float* row_skip, void* stream);

/* The music side of the sharded retrieval as ONE buffer for ONE all-gather (reference test-MaDe.py:386-403 over the 8 GPUs of a node): a
 * record per track, [S * D segment embeddings in pack_dtype | S mask floats | D floats of the pooled music vector | zero pad to rec_bytes
 * (a multiple of 16)].  seg [n, S, D] (f32 or bf16, track stride seg_bs elements, S * D contiguous), mask [n, S] f32, music [n, D] f32;
 * records n .. n_pad - 1 (the shards are padded to the largest) are zero-filled. */
int made_pack_music_records(const void* seg, int32_t seg_dtype, int64_t seg_bs, const float* mask, int64_t ld_mask, const float* music, int64_t ld_music,
                            void* out, int32_t pack_dtype, int64_t rec_bytes, int64_t n, int64_t n_pad, int64_t S, int64_t D, void* stream);

/* y[r, :] = x[r, :] * (mask[r] != 0) converted to y_dtype: the masked_fill of reference model/model_Base.py:556,595
 * fused with the f32 -> bf16 conversion of the pre-extracted features, so the input projection can use the
 * direct-to-LDS GEMM path.  mask may be NULL. */
int made_cast_mask_rows(const float* x, int64_t ldx, const float* mask, void* y, int32_t y_dtype, int64_t ldy,
                        int64_t rows, int64_t D, void* stream);

/* out[b, :] = sum_t x[b,t,:] * (mask[b,t] != 0) / sum_t mask[b,t]   (mask NULL: plain column sum,
 * no division).  Replaces reference model/model_Base.py:579,615 and the sum over frames inside
 * reference music_detr/loss_detr.py:116-117. */
int made_masked_mean(const void* x, int32_t x_dtype, int64_t x_bs, int64_t ldx, const float* mask,
                     float* out, int64_t B, int64_t T, int64_t D, void* stream);

/* y = x / max(||x||_2, eps) per row (F.normalize): reference model/model_Base.py:580,616,
 * model/model_Uni.py:142,146.  y_f32 and/or y_alt (dtype y_alt_dtype) may be NULL. */
int made_l2norm_rows(const void* x, int32_t x_dtype, int64_t ldx, float* y_f32, void* y_alt, int32_t y_alt_dtype,
                     int64_t ldy, int64_t rows, int64_t D, float eps, void* stream);

/* Mask-aware normalised sine position embedding: reference music_detr/position_encoding.py:51-71.
 * mask [B,L] f32; dim_t [D] f32 (= 10000^(2*floor(i/2)/D), computed once by the host exactly as the
 * reference does); out [B,L,D] in out_dtype. */
int made_sine_pe(const float* mask, const float* dim_t, void* out, int32_t out_dtype,
                 int64_t B, int64_t L, int64_t D, void* stream);

/* In-place-capable masked softmax over the last axis of logits [M_outer, R, S] (f32, row stride
 * lds_): p = softmax(logits*scale + (mask[m, s]==0 ? -inf : 0)); columns in [S, S_pad) are written
 * as 0.  Output dtype out_dtype, row stride ldp.  The softmax over segments ("clips") of the
 * X-Pool block: reference modules/transformer.py:110-117. */
int made_masked_softmax(const float* logits, int64_t ld_logits, const float* mask, int64_t ld_mask,
                        void* probs, int32_t out_dtype, int64_t ldp,
                        int64_t M_outer, int64_t R, int64_t S, int64_t S_pad, float scale, void* stream);

/* made_xpool_fused: all-pairs X-Pool scoring in one kernel (bf16, D = 256): for every (video n, track m)
 *   softmax_s(<Q[n], K[m,s]> * scale + mask) . U[m,s,:] -> LayerNorm2 -> x + (Wl x + bl) -> LayerNorm3 -> cosine with vn[n]
 *   -> sims[n*ld_sims + m].
 * Replaces, for retrieval (reference test-MaDe.py:392-403), the chain modules/transformer.py:110-123 (attention; out_proj is
 * hoisted onto the values by the caller: U = out_proj(v_proj(LN1(seg))), valid because the softmax rows sum to 1),
 * :172-178 (LayerNorm2, linear_proj with residual, LayerNorm3) and modules/metrics.py:19-24 (cosine) -- no [Nm*Nv, D]
 * tensor is ever written.  Q = q_proj(LN1(video)) [Nv, D]; K = k_proj(LN1(seg)), U [Nm, S, D] (rows at m*{k,u}_bs + s*ld);
 * key_mask [Nm, S] f32 or NULL; vn = video / |video| [Nv, D] f32.  A track with no valid segment gives NaN, like the
 * reference's softmax over -inf.  LayerNorm variances are taken in one pass (E[x^2] - E[x]^2, f32): a bf16-path kernel.
 * Rounding points (everything else is f32; tests/xpool_ref.py restates this list): the probabilities exp2(s - m) before the P.U product
 * (their denominator is the f32 sum of the unrounded ones); o^ = O / l before the Linear, AFTER LayerNorm2's sums were taken from the
 * f32 o^ (so k2 = -mean rstd belongs to the unrounded row: with value rows that share an offset the two no longer cancel, see
 * docs/EXPERIMENTS.md 3p); the folded weight W'' = (W + I) diag(g2) (Av, Bv are f32 sums over the given W); g3 vn in the cosine's
 * numerator (the per-video sums over g3 vn are f32). */
typedef struct MadeXpoolFusedArgs {
    const void* Q; int64_t ldq;
    const void* K; const void* U; int64_t k_bs, ldk, u_bs, ldu;
    const float* key_mask;
    const float* ln2_g; const float* ln2_b;
    const void* Wl; int64_t ldw; const float* bl;
    const float* ln3_g; const float* ln3_b;
    const float* vn; int64_t ldvn;
    float* sims; int64_t ld_sims;
    int64_t Nv, Nm, S, D;
    float scale, eps;
    float* ws;                 /* workspace, Nv*(D+2) + 4 + 2*D + D*D/2 + 4*Nm floats, 16-byte aligned: per-video terms of LayerNorm3 +
                                  cosine that do not depend on the track, the Linear folded with LayerNorm2 (bf16 weight, two
                                  vectors), four ints per track (valid range of its segments) */
    int32_t prepare_ws; int32_t _pad;   /* 1: fill the per-video and per-model parts of ws first (small launches); 0: they are still
                                           valid from a previous call with the same vn, ln2, Wl, bl and ln3 (the caller loops over
                                           chunks of tracks); the per-track part is rebuilt by every call */
} MadeXpoolFusedArgs;

int made_xpool_fused(const MadeXpoolFusedArgs* args, void* stream);

/* made_xpool_attention: the attention of the X-Pool block at retrieval scale (every video against the segments of every track, ONE head
 * of width D = 256 or 512; reference modules/transformer.py:87-123 as called by Transformer_XA.forward :156-180 and test-MaDe.py:392-395)
 * plus the normalisation of LayerNorm2 (:172) without its affine part:
 *   o[m, n, :]   = softmax_s(<Q[n], K[m, s]> * scale + (key_mask[m, s] == 0 ? -inf : 0)) . U[m, s, :]
 *   out[m, n, :] = normalize ? (o - mean(o)) * rsqrt(var(o) + eps) : o                       (bf16, row (m * Nv + n) * ldo)
 * The caller folds LayerNorm2's gamma / beta into the Linear that follows (W'' = (W + I) diag(gamma), b'' = (W + I) beta + b), so the
 * residual of modules/transformer.py:176 costs nothing.  Two passes per track with the probabilities parked in LDS (bf16), K / U rows
 * through LDS-DMA; S <= 512 segments.  Q [Nv, D], K / U [Nm, S, D] (rows at m * {k,u}_bs + s * ld{k,u}), all bf16; key_mask [Nm, S] f32
 * or NULL; ws: Nm * 32 ints (valid range and one bit per segment of every track), 16-byte aligned.  A track without a valid segment
 * gives NaN rows, like the reference's softmax over -inf.
 * Rounding points: the probabilities before the P.U product (denominator: the f32 sum of the unrounded ones) and the bf16 output rows;
 * mean and the one-pass variance are f32 sums over the f32 o. */
typedef struct MadeXpoolAttnArgs {
    const void* Q; int64_t ldq;
    const void* K; const void* U; int64_t k_bs, ldk, u_bs, ldu;
    const float* key_mask;
    void* out; int64_t ldo;
    int64_t Nv, Nm, S, D;
    float scale, eps;
    int32_t normalize; int32_t _pad;
    void* ws;
} MadeXpoolAttnArgs;

int made_xpool_attention(const MadeXpoolAttnArgs* args, void* stream);

/* made_xpool_sims: all-pairs X-Pool scoring with the per-pair Linear moved onto the values (round 4; D = 256, tracks of at most 96 segments).  The chain of
 * reference modules/transformer.py:156-180 + modules/metrics.py:10-24 after the attention is
 *   y = W'' xhat + b'',  xhat = (o - mean(o)) rstd(o),  W'' = (W + I) diag(g2), b'' = (W + I) b2 + b          (LayerNorm2 + Linear + residual)
 * and o = sum_s p_s u_s is a convex combination of the track's value rows, so W'' o = sum_s p_s (W'' u_s): with u''_s = W'' u_s made ONCE per
 * segment by a GEMM over the tracks (the caller: columns [D, 2D) of the value rows), the per-pair 2 D^2 flops of the Linear become a second
 * P.V product of 2 S D flops, and   y = k1 (P.U'') + k2 Bv + Av,   k1 = rstd(o), k2 = -mean(o) rstd(o), Av = b'', Bv = W'' 1.
 * LayerNorm3 and the cosine with the video are the six sums of made_xpool_fused; nothing per pair is written but sims[n * ld_sims + m].
 * Q [Nv, D] bf16; K [Nm, S, D] bf16 (rows at m * k_bs + s * ldk); UU [Nm, S, 2 D] bf16 (rows at m * u_bs + s * ldu: u_s | u''_s);
 * key_mask [Nm, S] f32 or NULL; av, bv, ln3_g, ln3_b [D] f32; vn = video / |video| [Nv, D] f32; ws: made_xpool_sims_ws_bytes(Nv, Nm, D)
 * bytes, 16-byte aligned (per-video terms of LayerNorm3 + cosine -- since round 5 with a second, bf16 copy of g3 * vn in the order the 64-video kernel's lanes
 * read it; Nv * ldq * 2 and Nv * (1.5 D + 4) * 4 must stay below 4 GB -- filled when prepare_ws != 0; 32 ints per track, rebuilt by every call).
 * Two kernels serve the call: 32 videos per workgroup (the default) and 64 (MADE_XPOOL_SIMS_PQ=64: the same sums in the same order, results equal to 1e-7).
 * A track without a valid segment gives NaN, like the reference's softmax over -inf.
 * Rounding points of both kernels (everything else is f32): the probabilities before the two P.V products (denominator: the f32 sum of the
 * unrounded ones; LayerNorm2's sums are taken from the f32 o); g3 vn in the sum over g3 vn z; and the seven sums that are LINEAR in z --
 * sum z c for c = 1, Bv, Av, g3^2, g3^2 Bv, g3^2 Av, g3 b3 -- go through the matrix pipe: there z (before the division by l: values of at
 * most max|u''|) AND the seven constant vectors are bf16.  The sums over z^2 and the per-model / per-video constants are f32. */
typedef struct MadeXpoolSimsArgs {
    const void* Q; int64_t ldq;
    const void* K; const void* UU; int64_t k_bs, ldk, u_bs, ldu;
    const float* key_mask;
    const float* av; const float* bv;
    const float* ln3_g; const float* ln3_b;
    const float* vn; int64_t ldvn;
    float* sims; int64_t ld_sims;
    int64_t Nv, Nm, S, D;
    float scale, eps;
    void* ws;
    int32_t prepare_ws; int32_t _pad;
} MadeXpoolSimsArgs;

int     made_xpool_sims(const MadeXpoolSimsArgs* args, void* stream);
int64_t made_xpool_sims_ws_bytes(int64_t Nv, int64_t Nm, int64_t D);

/* made_xpool_sims_pairs: made_xpool_sims for LISTED pairs (the second stage of `ground(..., shortlist=R)`: bf16, D = 256, S <= 96).  The pairs are
 * a CSR over U tracks: pair p in [start[u], start[u + 1]) is (video[p], track u), start [U + 1] ascending, the videos of a track in any order
 * (the caller lists them ascending); score [P] f32 receives the X-Pool similarity of every pair.  K [U, S, D], UU [U, S, 2 D] = u | u'',
 * key_mask [U, S] or NULL, av, bv, ln3_g, ln3_b, vn and Q as for made_xpool_sims -- the same arithmetic: scores by MFMA, masked softmax in f32,
 * probabilities rounded to bf16 before the two P.V products, y = k1 z + k2 Bv + Av, LayerNorm3 and the cosine through the six sums in f32;
 * rounding points differ from made_xpool_sims (z and g3 vn stay f32), results agree to the bf16 bound, not bit for bit.  One workgroup per
 * track and tile of 32 listed videos; the track's value rows go through LDS once per workgroup, Q rows and vn rows are gathered by video
 * index; no workspace, no preparation launch, no atomics.  A pair's result does not depend on the other pairs of the launch or of its tile.
 * A track without a valid segment gives NaN; a video index outside [0, Nv) gives NaN and nothing is read for it; an empty range is legal;
 * start values are clamped to [0, P].  max_count: the longest range (sizes the grid; 0 or an underestimate only costs speed). */
typedef struct MadeXpoolPairsArgs {
    const void* Q; int64_t ldq;
    const void* K; const void* UU; int64_t k_bs, ldk, u_bs, ldu;
    const float* key_mask;
    const float* av; const float* bv;
    const float* ln3_g; const float* ln3_b;
    const float* vn; int64_t ldvn;
    const int32_t* start; const int32_t* video;
    float* score;
    int64_t Nv, U, P, S, D, max_count;
    float scale, eps;
} MadeXpoolPairsArgs;

int     made_xpool_sims_pairs(const MadeXpoolPairsArgs* args, void* stream);

/* made_xpool_inbatch: the in-batch X-Pool contraction for a batch of at most 64 videos -- out[m, n, :] = softmax_s(scale q_n . k_{m,s} + mask) U_m
 * (reference modules/transformer.py:110-119, out projection hoisted onto the values; the north-star contraction).  Two launches of one
 * workgroup per CU -- scores per (track, 128 segments) with the tile-local softmax pieces, then P.V per (track, 128 value columns) -- with only
 * the bf16 probabilities between them; replaces made_attention_wide's key split + merge on this shape.  Q [Nv <= 64, D], K / U [Nm, S <= 512, D]
 * (rows at m * {k,u}_bs + s * ld{k,u}), bf16, D = 256 / 512; key_mask [Nm, S] f32 or NULL; out[m * o_bs + n * ldo + d] bf16 or f32;
 * ws: made_xpool_inbatch_ws_bytes(Nm, S) bytes, 16-byte aligned (a larger workspace may be reused for a smaller call).  A track without a valid
 * segment gives NaN rows (the reference's softmax).  Rounding points: per 32-segment tile p~ = exp2(s - ceil(tile maximum)) in bf16 (the
 * denominator sums the ROUNDED p~, in f32); a tile's p~ is brought to the track's reference by an exact power of two 2^-k, k clamped to 255,
 * on the bf16 exponent field: a value that leaves the normal range becomes +0 or a bf16 subnormal (weight below 2^-126); the output rows when bf16.
 * (Round 5's opt-in one-launch form -- both roles in one workgroup, the probabilities handed
 * over inside the launch -- was 4 % faster alone and is gone: docs/EXPERIMENTS.md.) */
typedef struct MadeXpoolInbatchArgs {
    const void* Q; int64_t ldq;
    const void* K; const void* U; int64_t k_bs, ldk, u_bs, ldu;
    const float* key_mask;
    void* out; int32_t out_dtype; int32_t _pad; int64_t o_bs, ldo;
    int64_t Nv, Nm, S, D;
    float scale; int32_t _pad2;
    void* ws;
} MadeXpoolInbatchArgs;

int     made_xpool_inbatch(const MadeXpoolInbatchArgs* args, void* stream);
int64_t made_xpool_inbatch_ws_bytes(int64_t Nm, int64_t S);

/* How made_xpool_sims / made_xpool_fused / made_xpool_attention cut these arguments into workgroups: the launch calls the same function, so
 * the answer IS the dispatch.  Returns MADE_OK or the status with which the launch would refuse the arguments; nothing is launched and no
 * pointer is dereferenced (their alignment is looked at), so the question can be asked without a GPU.  Nv == 0 or Nm == 0 (nothing is
 * launched) reports chunks = 0.  Measurement knobs (honoured under MADE_DEBUG_VARIANTS only): MADE_XPOOL_SIMS_PQ=64 the 64-video kernel;
 * MADE_XPOOL_SIMS_PER / MADE_XPOOL_FUSED_PER / MADE_XPOOL_ATTN_PER = n > 0: exactly n tracks per chunk (clamped to the kernel's track
 * table: 464 / 440 for the 32- / 64-video sims kernel, 1024 for made_xpool_fused; to Nm for made_xpool_attention, which has none). */
enum MadeXpoolKernel {
    MADE_XPOOL_KERNEL_SIMS32 = 0,   /* xpool_sims32_kernel: 32 videos, four waves, two workgroups per CU */
    MADE_XPOOL_KERNEL_SIMS64 = 1,   /* xpool_sims64_kernel: 64 videos (MADE_XPOOL_SIMS_PQ=64) */
    MADE_XPOOL_KERNEL_FUSED = 2,    /* xpool_fused_persist_kernel: 64 videos, attention + linear waves */
    MADE_XPOOL_KERNEL_ATTN256 = 3,  /* xpool_attn_kernel<256> */
    MADE_XPOOL_KERNEL_ATTN512 = 4   /* xpool_attn_kernel<512> */
};
typedef struct MadeXpoolPlan {
    int32_t kernel;             /* MadeXpoolKernel */
    int32_t videos_per_wg;      /* 32 or 64 */
    int32_t video_tiles;        /* ceil(Nv / videos_per_wg) */
    int32_t tracks_per_chunk;   /* tracks a workgroup walks (the last chunk may be shorter) */
    int32_t chunks;             /* chunks that hold a track: ceil(Nm / tracks_per_chunk) */
    int32_t chunks_launched;    /* >= chunks: made_xpool_sims pads to a multiple of 8 from 8 chunks on (the padded workgroups exit at once) */
    int32_t xcd_order;          /* 1: chunk c is walked by the workgroups of XCD c % 8 (made_xpool_sims with chunks_launched % 8 == 0) */
    int32_t _pad;
} MadeXpoolPlan;
int made_xpool_sims_plan(const MadeXpoolSimsArgs* args, MadeXpoolPlan* plan);
int made_xpool_fused_plan(const MadeXpoolFusedArgs* args, MadeXpoolPlan* plan);
int made_xpool_attention_plan(const MadeXpoolAttnArgs* args, MadeXpoolPlan* plan);

/* made_row_affine: out[r, :] = act(x[r, :] * scale[r % period] + shift[r % period]), act = none | ReLU.  Eval-mode
 * BatchNorm1d of the EmbeddingNet aggregator (reference model/model_Base.py:224-229): its input is [B, T, F], so the
 * "channels" are the T token positions and the running statistics reduce to one (scale, shift) per position. */
int made_row_affine(const void* x, int32_t x_dtype, int64_t ldx, const float* scale, const float* shift, int64_t period,
                    int32_t act, void* out, int32_t out_dtype, int64_t ldo, int64_t rows, int64_t cols, void* stream);

/* X-Pool tail: y [Nm*Nv, D] (the pre-LayerNorm3 sum, reference modules/transformer.py:177) ->
 * LayerNorm3 -> (optional) pooled[m,n,:] -> cosine with video n -> sims[n*ld_sims + m].
 * Fuses reference modules/transformer.py:178 with modules/metrics.py:19-24 so the pooled tensor
 * need not be materialised.  video [Nv,D] f32. */
int made_xpool_tail(const void* y, int32_t y_dtype, int64_t ldy, const float* gamma, const float* beta,
                    const float* video, int64_t ld_video, float* pooled_out /* [Nm*Nv,D] or NULL */,
                    float* sims, int64_t ld_sims, int64_t Nm, int64_t Nv, int64_t D, float eps, void* stream);

/* Symmetric cross-entropy of reference modules/loss.py:5-24 (== InfoNCELoss with audio_id=None,
 * :116-122): loss_out[0] (+)= weight * 0.5*(CE_rows + CE_cols) of sims*exp(*logit_scale).
 * accumulate != 0 adds to loss_out[0] instead of overwriting.  n <= 4096. */
/* row_exclude [n, n] f32 or NULL (made_clip_loss and made_clip_loss_bwd): entries equal to 1 are left out of the row-direction
 * (video -> music) softmax -- the negatives that share the row's own music track when the drivers run with
 * --ignore_same_music 0 (reference modules/loss.py:90-114); the column direction always uses every entry. */
int made_clip_loss(const float* sims, int64_t ld, int64_t n, const float* logit_scale, float weight,
                   int32_t accumulate, float* loss_out, const float* row_exclude, void* stream);

/* ------------------------------------------------------------------------------------------
 * Hungarian matcher and set criterion (reference music_detr/matcher.py:36-92, loss_detr.py).   */

/* Cost + assignment for NS = n_layers*B independent samples (sample s uses targets[s % B]).
 *   pred_logits [NS,Q,2] f32, pred_spans [NS,Q,2] f32 (centre,width), targets [B,G,2] f32;
 *   targets with width == 0 are dropped (reference matcher.py:59-61) and tgt indices refer to the
 *   kept targets in order.  cost = w_span*L1 + w_giou*(-GIoU) + w_class*(-softmax(logits)[fg]) in
 *   f32, evaluated left to right without FMA contraction (reference matcher.py:88); the assignment
 *   is SciPy's rectangular LSAP on the f64-promoted block (reference matcher.py:91), same tie-break.
 *   cost_ws [NS,Q,G] f32 workspace (holds the per-sample cost blocks on return).  With
 *   cost_is_input != 0 the cost step is skipped and cost_ws is taken as given (block of sample s =
 *   cost_ws[s, :Q, :kept targets of s]); used to check the assignment bit-for-bit on identical costs:
 *   the class term goes through exp(), whose last bit differs between libms, and a 1-ulp change can
 *   flip an assignment whose two best solutions tie to ~1e-7 (both are then optimal).
 *   out_pred_idx/out_tgt_idx [NS, min(Q,G)] int64, rows ascending in pred index, unused = -1;
 *   out_count [NS] int32; status [1] int32: 0, or 1 if any cost was NaN/-inf or infeasible
 *   (SciPy raises ValueError there).  Q, G <= 64. */
int made_hungarian_match(const float* pred_logits, const float* pred_spans, const float* targets,
                         int64_t NS, int64_t B, int64_t Q, int64_t G, int32_t fg_label,
                         float w_span, float w_giou, float w_class,
                         float* cost_ws, int32_t cost_is_input, int64_t* out_pred_idx, int64_t* out_tgt_idx,
                         int32_t* out_count, int32_t* status, void* stream);

/* Set criterion for `n_layers` decoder layers at once (reference music_detr/loss_detr.py:74-169):
 *   losses [n_layers, 5] f32 = {loss_span, loss_giou, loss_label, class_error, loss_contrastive_align}
 *   per layer, and *total = sum_l sum_k weights[k]*losses[l,k] (class_error has weight 0).
 *   proj_queries [n_layers,B,Q,Dc] f32 and vid_sum [B,Dc] f32 (= sum over frames of proj_vid_mem)
 *   may be NULL (no contrastive term).  empty_weight [2] f32. */
int made_set_criterion(const float* pred_logits, const float* pred_spans, const float* targets,
                       const int64_t* pred_idx, const int64_t* tgt_idx, const int32_t* count,
                       const float* proj_queries, const float* vid_sum, const float* empty_weight,
                       int64_t n_layers, int64_t B, int64_t Q, int64_t G, int64_t Dc, int32_t fg_label,
                       float temperature, const float* weights /* [5] */,
                       float* losses, float* total, void* stream);


/* ==========================================================================================
 * Training path (backward kernels).  The reference trains through torch autograd
 * (reference train-MaDe.py:337-381: forward, loss.backward(), three clip_grad_norm_, Adam); the
 * entries below are the hand-written counterparts of the autograd nodes on the hot path.
 * ========================================================================================== */

/* made_attention_bwd: gradients of made_attention (flash style: the probabilities are recomputed from Q, K and the saved
 * log-sum-exp; nothing of size Lq x Lk touches HBM).  With Pd = dropout(P):
 *   delta_i = dO_i . O_i      dV = Pd^T dO      dP = dropout'(dO V^T)      dS = P * (dP - delta)
 *   dQ = scale * dS K         dK = scale * dS^T Q
 * Replaces autograd through nn.MultiheadAttention (reference model/model_Base.py:87, music_detr/transformer.py:199,287,
 * 293-296).  All tensors use the addressing of made_attention (element (b,i,h,d) at base + b*bs + i*ld + h*hd + d); dQ, dK,
 * dV may be column blocks of one [rows, 3*H*hd] buffer.  `delta` is a [B,H,Lq] f32 workspace the call fills (bf16: by the dQ kernel, for the
 * dK / dV kernel behind it; f32: by a launch of its own).  Rows of dQ
 * whose q_skip_mask is 0 and rows of dK/dV whose key_mask is 0 are written as zeros.  The per-sample mask / log-sum-exp / delta
 * rows live in LDS for the duration of a workgroup: MADE_ERR_UNSUPPORTED beyond ~8 000 queries or ~24 000 keys (fewer at
 * f32 head dim 128). */
typedef struct MadeAttnBwdArgs {
    const void* Q; const void* K; const void* V; const void* O; const void* dO;
    void* dQ; void* dK; void* dV;
    const float* lse; float* delta;
    int32_t dtype; int32_t hd;
    int64_t B, H, Lq, Lk;
    int64_t q_bs, ldq, k_bs, ldk, v_bs, ldv, o_bs, ldo, do_bs, lddo, dq_bs, lddq, dk_bs, lddk, dv_bs, lddv;
    const float* key_mask; const float* q_skip_mask;
    float scale; int32_t f32_products;   /* 0 = exact f32 products, 1 = split-bf16 (see "f32 products" above) */
    MadeDropout drop;
    const int32_t* batch_order; /* [B] or NULL: issue order of the batch, as in MadeAttnArgs */
    const uint32_t* keep_bits; int64_t ld_bits;   /* NULL, or the forward's dropout decisions (MadeAttnArgs.keep_bits; bf16 path): the
                                                     same mask as re-drawing it, bit for bit */
} MadeAttnBwdArgs;

int made_attention_bwd(const MadeAttnBwdArgs* args, void* stream);

/* made_gemm_tn: C[N,K] (+)= alpha * sum_m A[m,n] * B[m,k]   (reduction index m is the slow dimension of both operands).
 * The weight gradient of every nn.Linear on the path: dW = dY^T X with A = dY [M,N], B = X [M,K], and
 * colsum[n] += alpha * sum_m A[m,n] is the bias gradient.  Also the P^T dO / dS^T Q products of the wide-head attention
 * backward (batched).  Batch index z = z1 * batch2 + z2 with independent element strides per level (a C stride of 0 sums
 * the batch into one C).  split_m > 1 splits the reduction over workgroups; partial tiles are combined with f32 atomic
 * adds, so it requires accumulate = 1 and an f32 C that the caller has initialised (gradients are zeroed once per step).
 * Rows whose row_mask is 0 are read as zero in BOTH operands (padded tokens may hold stale data).
 * M == 0 adds nothing and stores nothing (C is not cleared, whatever `accumulate` says), and so does an EMPTY ROW LIST (*n_rows == 0),
 * in every kernel of made_gemm_tn and made_gemm_tn_grouped: callers zero gradients once per step.  (A row mask that is zero
 * everywhere is a reduction over M rows of zeros: a plain store then writes zeros.) */
typedef struct MadeGemmTNArgs {
    const void* A; const void* B; void* C;
    int32_t ab_dtype; int32_t c_dtype;             /* MadeDtype; C is f32 or the operand dtype */
    int64_t M, N, K;
    int64_t lda, ldb, ldc;
    int64_t batch1, batch2;
    int64_t a_zs1, a_zs2, b_zs1, b_zs2, c_zs1, c_zs2;
    const float* row_mask; int64_t mask_zs1, mask_zs2;
    float   alpha; int32_t accumulate;
    int64_t split_m;
    float*  colsum; int64_t colsum_zs1, colsum_zs2; /* optional, always accumulated */
    const float* row_group_valid;                   /* optional [ceil(M/32)] (made_row_groups of row_mask; unbatched calls): slabs
                                                       whose rows are all masked are skipped without being loaded */
    const int32_t* row_index; const int32_t* n_rows; /* optional row gather (unbatched calls): the reduction runs over the
                                                       *n_rows rows row_index[0..] only (made_row_index); row_mask is not needed */
    int32_t f32_products; int32_t _pad;             /* 0 = exact f32 products, 1 = split-bf16 (see "f32 products" above) */
} MadeGemmTNArgs;

int made_gemm_tn(const MadeGemmTNArgs* args, void* stream);

/* Which kernel made_gemm_tn dispatches these arguments to, or the (negative) MadeStatus with which made_gemm_tn would refuse them.
 * Nothing is launched and no pointer is dereferenced (the pointers' alignment is looked at), so the question can be asked without a GPU.
 * M == 0, which launches nothing, reports the tiled kernel of its dtype. */
enum MadeGemmTNVariant {
    MADE_GEMM_TN_SMALL = 0,        /* gemm_tn_small_kernel: one thread per C element; operands that 16-byte chunks cannot address */
    MADE_GEMM_TN_TILED_BF16 = 1,   /* gemm_tn_kernel<bf16>: 128 x 128 tiles, register-staged slabs of 64 rows, every option */
    MADE_GEMM_TN_TILED_F32 = 2,    /* gemm_tn_kernel<float>: slabs of 32 rows, exact f32 products */
    MADE_GEMM_TN_TILED_F32X3 = 3,  /* gemm_tn_kernel<float, X3>: the same with split-bf16 products (f32_products = 1) */
    MADE_GEMM_TN_GLDS = 4          /* gemm_tn_glds_kernel: bf16, N and K multiples of 128, unbatched, M >= 256, no row mask (or a row list),
                                      at most 4096 rows per workgroup: slabs go global -> LDS directly */
};
int made_gemm_tn_variant(const MadeGemmTNArgs* args);

/* made_gemm_tn_grouped: up to 8 weight gradients that reduce over the same rows -- the Linears of one transformer layer
 * (reference music_detr/transformer.py:191-210, model/model_Base.py:64-91: dW_i += alpha * dY_i^T X_i, db_i += alpha * colsum(dY_i)) --
 * in ONE launch: bf16 operands, f32 C accumulated (with atomics, or through the workspace below; the caller zeroes gradients once per step), N_i and K_i multiples
 * of 128, one row list (row_index / n_rows as in made_gemm_tn, or all M rows) and one split of the reduction for all problems.
 * tile_end is filled in by the library. */
#define MADE_GEMM_TN_MAX_GROUP 8
typedef struct MadeGemmTNProblem {
    const void* A; const void* B; float* C; float* colsum;      /* A [M, N] = dY, B [M, K] = X, C [N, K], colsum [N] or NULL */
    int64_t N, K, lda, ldb, ldc;
} MadeGemmTNProblem;
typedef struct MadeGemmTNGroup {
    int32_t n_problems; float alpha;
    int64_t M, split_m;
    const int32_t* row_index; const int32_t* n_rows;
    MadeGemmTNProblem p[MADE_GEMM_TN_MAX_GROUP];
    int32_t tile_end[MADE_GEMM_TN_MAX_GROUP];
    int32_t tile_size; int32_t _pad;     /* 0 / 128: 128 x 128 output tiles (four waves, two workgroups per CU); 256: 256 x 256 tiles (eight waves, one
                                            workgroup per CU, N and K multiples of 256, M <= 36864): twice the flops per operand byte, a quarter of
                                            the atomics; the (tile, 64-row slab) units are cut into equal ranges for the workgroups, split_m is not used */
    void* workspace; int64_t workspace_bytes;   /* optional, 256 x 256 tiles only (ABI 8): with it the workgroups that share a tile's reduction STORE their f32
                                            partials there and a second launch of the same call sums them in a fixed order and updates C with plain
                                            accesses -- instead of adding every partial to C with atomics (67 MB of atomic adds per encoder layer at the
                                            1.2 TB/s the atomic units sustain: 83 of the launch's 146 us).  At least
                                            made_gemm_tn_grouped_workspace(group) bytes, 16-byte aligned, contents arbitrary; calls that share a
                                            workspace, or update the same C, must be ordered on one stream.  The result is then bitwise
                                            reproducible.  NULL: the atomics.  A group whose need reaches 2^32 bytes (the first launch addresses its
                                            slots with 32-bit offsets; eight problems of 4096 x 4096 at M = 36864 need 4.36e9) is MADE_ERR_UNSUPPORTED
                                            with a workspace: pass NULL for it */
} MadeGemmTNGroup;
int made_gemm_tn_grouped(const MadeGemmTNGroup* group, void* stream);
/* bytes of workspace the group's launch can use (0: none -- not the 256 x 256-tile form); reads n_problems, tile_size, M and the problems' N, K */
int64_t made_gemm_tn_grouped_workspace(const MadeGemmTNGroup* group);
/* out[g] = 1 if any of mask[32g .. 32g+31] is nonzero else 0 (computed once per batch, shared by every weight-gradient product) */
int made_row_groups(const float* mask, int64_t M, float* out, void* stream);
/* made_row_index: compaction of a [M] token mask: row_index[r] = index of the r-th nonzero entry (r < n), entries r >= n repeat
 * the last valid row (0 when there is none), n_rows[0] = n.  One workgroup, M <= 2^22.  Feeds the row gather of made_linear /
 * made_gemm_tn: the GEMMs of a padded batch then cost what its valid tokens cost. */
int made_row_index(const float* mask, int64_t M, int32_t* row_index, int32_t* n_rows, void* stream);
/* made_batch_order: order[r] = index of the sample with the r-th largest number of nonzero mask entries (mask [B, T]; ties in
 * ascending sample index, so the result is a deterministic permutation).  The `batch_order` of made_attention / _bwd.
 * One workgroup, B <= 8192. */
int made_batch_order(const float* mask, int64_t B, int64_t T, int32_t* order, void* stream);

/* Row kernels of the backward pass (all parameter gradients are ACCUMULATED into f32 buffers the caller zeroes once per step).
 *
 * made_layernorm_bwd: dx = LN'(x; gamma)(dy) [+ add]; optionally also dx_drop = dropout(dx) (the gradient entering a
 *   residual branch whose output was dropped: `x + dropout(branch)`); dgamma += sum dy*xhat, dbeta += sum dy.  Rows whose
 *   row_skip is 0 are neither read nor written and contribute nothing (their consumers gather / mask the valid rows).  Autograd of nn.LayerNorm at reference model/model_Base.py:77-78,
 *   music_detr/transformer.py:157-158,235-237, modules/transformer.py:141-143. */
int made_layernorm_bwd(const void* x, int32_t x_dtype, int64_t ldx, int64_t x_rows_per_batch, int64_t x_batch_stride,
                       const float* gamma, const void* dy, int32_t dy_dtype, int64_t lddy,
                       const void* add, int32_t add_dtype, int64_t ld_add,
                       void* dx, int32_t dx_dtype, int64_t lddx,
                       void* dx_drop, int64_t lddxd, const MadeDropout* drop, int64_t drop_ld,
                       float* dgamma, float* dbeta, int64_t rows, int64_t D, float eps, const float* row_skip, void* stream);

/* made_pool_bwd: backward of vec = normalize(masked_mean(local)) (reference model/model_Base.py:579-580,615-616) merged with
 *   the other gradients of `local`: out[b,t,:] = mask[b,t] * (in1[b,t,:] + in2[b,t,:] + dmean[b,:] / count_b),
 *   dmean = (dvec - vhat (vhat.dvec)) / |mean|, and dvec / eps where |mean| < eps (F.normalize's clamp divides by a constant:
 *   no projection term).  in1 / in2 may be NULL. */
int made_pool_bwd(const float* mean, const float* dvec, const float* mask,
                  const void* in1, int32_t in1_dtype, int64_t in1_bs, int64_t in1_ld,
                  const void* in2, int32_t in2_dtype, int64_t in2_bs, int64_t in2_ld,
                  void* out, int32_t out_dtype, int64_t out_bs, int64_t out_ld,
                  int64_t B, int64_t T, int64_t D, float eps, void* stream);

/* made_l2norm_bwd: y = x / max(|x|, eps)  ->  dx = (dy - yhat (yhat.dy)) / |x|, and dy / eps where |x| < eps; dx f32 (stored or accumulated)
 *   and/or dx_alt in another dtype (always the plain gradient).  dy row of x row r is r / dy_rows_per (0 or 1: one each).  F.normalize at reference model/model_Uni.py:142-146, cosine at modules/loss.py:52-56. */
int made_l2norm_bwd(const void* x, int32_t x_dtype, int64_t ldx, const float* dy, int64_t lddy, int64_t dy_rows_per,
                    float* dx, int64_t lddx, int32_t accumulate, void* dx_alt, int32_t alt_dtype, int64_t lddxa,
                    int64_t rows, int64_t D, float eps, void* stream);

/* made_clip_loss_bwd: gradient of weight * CLIPLoss(sims, logit_scale) (reference modules/loss.py:5-24) times upstream[0]
 *   (NULL = 1): dsims [n,n] and its transpose dsims_t (may be NULL), d_logit_scale[0] += .  lse_ws: [2n] f32 workspace. */
int made_clip_loss_bwd(const float* sims, int64_t ld, int64_t n, const float* logit_scale, float weight,
                       const float* upstream, float* lse_ws, float* dsims, float* dsims_t, int32_t accumulate,
                       float* d_logit_scale, const float* row_exclude, void* stream);

/* made_xpool_tail_bwd: backward of made_xpool_tail (LayerNorm3 + cosine with the video, reference modules/transformer.py:178,
 *   modules/metrics.py:10-24): dy [Nm*Nv, D], optionally dy_drop = dropout(dy) (element index row*D + col), dgamma/dbeta
 *   accumulated, dvideo[n,:] += (atomic).  dpool [Nm, D] f32 or NULL: an additional gradient of the pooled rows themselves,
 *   dpool[m, :] * dpool_scale for every n (moment_query_type = "xpool": the decoder's content query is the mean over the
 *   videos of a track's pooled vectors, reference model/model_Uni.py:222-223). */
int made_xpool_tail_bwd(const void* y, int32_t y_dtype, int64_t ldy, const float* gamma, const float* beta,
                        const float* video, int64_t ld_video, const float* dsims, int64_t ld_dsims,
                        void* dy, int32_t dy_dtype, int64_t lddy, void* dy_drop, const MadeDropout* drop,
                        float* dgamma, float* dbeta, float* dvideo, int64_t ld_dvideo,
                        const float* dpool, int64_t ld_dpool, float dpool_scale,
                        int64_t Nm, int64_t Nv, int64_t D, float eps, void* stream);

/* made_softmax_bwd: softmax backward of the wide-head attention with materialised scores (few query rows per batch):
 *   P = softmax(scale*S + mask), Pd = dropout(P), dP = dropout'(dPd + extra[row]), dS = scale * P * (dP - sum_k P_k dP_k).
 *   Writes Pd and dS [rows, ldo] (columns L..ldo-1 zero, for any ldo >= L) and dS^T [rows/rows_per_batch, L, ldt] in out_dtype; the products
 *   dV = Pd^T dO, dK = dS^T Q and dQ = dS K are then made_gemm_tn calls.  mask row = row / rows_per_mask. */
int made_softmax_bwd(const float* S, int64_t ld_s, const float* dP, int64_t ld_dp, const float* mask, int64_t rows_per_mask,
                     const float* extra, float scale, const MadeDropout* drop,
                     void* Pd, void* dS, void* dSt, int32_t out_dtype, int64_t ldo, int64_t ldt,
                     int64_t out_batch_stride, int64_t t_batch_stride,   /* 0: dense (rows_per_batch*ldo, L*ldt) */
                     int64_t rows, int64_t rows_per_batch, int64_t L, void* stream);

/* x[row, h*hd + j] += s[row, h] * bias[h*hd + j]: the value-projection bias of the memory-space cross-attention when the
 * attention weights of a row no longer sum to 1 (dropout); s = that sum.  And its backward. */
int made_head_bias(void* x, int32_t x_dtype, int64_t ldx, const float* s, const float* bias, int64_t rows, int64_t H, int64_t hd,
                   void* stream);
int made_head_bias_bwd(const void* dy, int32_t dtype, int64_t ld, const float* s, const float* bias, float* dbias, float* ds,
                       int64_t rows, int64_t H, int64_t hd, void* stream);

/* made_layernorm_bwd2: two chained LayerNorms backward in one pass -- the decoder layer's norm 3 followed by the shared output norm
 * (reference music_detr/transformer.py:306 and :136): with t3 = LN_a(xa) and hs = LN_b(xb = the saved t3),
 *   g = LN_b'(dy) + add,  dx = LN_a'(g),  dx_drop = dropout(dx)  (element index row * drop_ld + col);
 * dgamma / dbeta of both norms are accumulated.  All row tensors share `dtype`; D <= 1024. */
int made_layernorm_bwd2(const void* xa, const float* gamma_a, int64_t ldxa, const void* xb, const float* gamma_b, int64_t ldxb,
                        const void* dy, int64_t lddy, const void* add, int64_t ld_add, void* dx, int64_t lddx,
                        void* dx_drop, int64_t lddxd, const MadeDropout* drop, int64_t drop_ld, int32_t dtype,
                        float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b, int64_t rows, int64_t D, float eps,
                        void* stream);

/* made_gate_rows: out[r, c] = dropout(x[r, c] * act'(G[r, c]) * scale)  (element index of the dropout r*drop_ld + c/drop_col_div,
 * drop_col_div <= 0 meaning 1: with drop_col_div = head width and drop_ld = H the mask is one draw per (row, head) -- the
 * attention-weight dropout of a self-attention over a single key, whose only weight is 1; rows whose row_skip is 0 are left
 * untouched).  The element-wise options of a made_linear epilogue for the places of the backward chain
 * where no GEMM can carry them: the activation after the input projection (reference model/model_Base.py:559-561, whose
 * input needs no gradient) and a residual stream that enters a dropped branch (temporal blocks deeper than one layer). */
int made_gate_rows(const void* x, int32_t x_dtype, int64_t ldx, const void* G, int32_t g_dtype, int64_t ldg, int32_t gate,
                   float scale, const MadeDropout* drop, int64_t drop_ld, int64_t drop_col_div, void* out, int32_t out_dtype, int64_t ldo,
                   const float* row_skip, int64_t rows, int64_t cols, void* stream);
/* out = a + b + c over n contiguous elements (b, c may be NULL; any mix of f32 / bf16): merges gradient streams.
 * b_mod > 0: b is broadcast, b[i % b_mod] (the decoder's query embedding added to every sample). */
int made_add3(void* out, int32_t out_dtype, const void* a, int32_t a_dtype, const void* b, int32_t b_dtype,
              const void* c, int32_t c_dtype, int64_t n, int64_t b_mod, void* stream);
/* out[c] += sum over rows of x[row, c]  (f32, accumulated): gradient of a row vector that was broadcast over the rows. */
int made_colsum(const void* x, int32_t dtype, int64_t ld, int64_t rows, int64_t cols, float* out, void* stream);

/* made_posbn_relu_fwd / _bwd: y = relu(BatchNorm1d_over_positions(x)) of the EmbeddingNet aggregator (agg_module = "mlp", reference
 *   model/model_Base.py:216-249: nn.BatchNorm1d(num_features = T) applied to [B, T, F], so position t is the channel and its
 *   statistics run over the B * F values there).  x / y: rows b * T + t of pitch ldx / ldy, F columns.  batch_stats != 0
 *   (model.train()): biased batch statistics normalise, running_mean / running_var (may both be NULL) move by `momentum` towards
 *   the batch mean / unbiased variance; batch_stats == 0 (model.eval()): the running statistics normalise.  save_mean /
 *   save_rstd [T] keep what was used, for the backward.  _bwd: dx (stored), dweight[t] += , dbias[t] += (may be NULL). */
int made_posbn_relu_fwd(const void* x, int32_t x_dtype, int64_t ldx, const float* weight, const float* bias,
                        float* running_mean, float* running_var, float momentum, float eps, int32_t batch_stats,
                        float* save_mean, float* save_rstd, void* y, int32_t y_dtype, int64_t ldy,
                        int64_t B, int64_t T, int64_t F, void* stream);
int made_posbn_relu_bwd(const void* x, int32_t x_dtype, int64_t ldx, const void* y, int32_t y_dtype, int64_t ldy,
                        const void* dy, int32_t dy_dtype, int64_t lddy, const float* weight, const float* save_mean,
                        const float* save_rstd, int32_t batch_stats, void* dx, int32_t dx_dtype, int64_t lddx,
                        float* dweight, float* dbias, int64_t B, int64_t T, int64_t F, void* stream);

/* made_set_criterion_bwd: gradients of made_set_criterion's total (times upstream[0]) w.r.t. pred_logits, pred_spans
 *   [n_layers,B,Q,2], proj_queries [n_layers,B,Q,Dc] (stored) and vid_sum [B,Dc] (accumulated).  d_logits / d_spans rows have
 *   pitch ld_out >= 2 (only columns 0,1 are written: a zero-padded pitch of 8 lets the row feed made_linear as an A operand);
 *   through_sigmoid != 0: d_spans is the gradient w.r.t. the pre-sigmoid value (pred_spans = sigmoid(z), model_Uni.py:135). */
int made_set_criterion_bwd(const float* pred_logits, const float* pred_spans, const float* targets,
                           const int64_t* pred_idx, const int64_t* tgt_idx, const int32_t* count,
                           const float* proj_queries, const float* vid_sum, const float* empty_weight,
                           int64_t n_layers, int64_t B, int64_t Q, int64_t G, int64_t Dc, int32_t fg_label,
                           float temperature, const float* weights, const float* upstream,
                           float* d_logits, float* d_spans, int64_t ld_out, int32_t through_sigmoid,
                           float* d_proj_queries, float* d_vid_sum, void* stream);

/* made_adam_step: the optimizer tail of one training iteration on the flat f32 master buffer (reference train-MaDe.py:
 * 262-266,375-381): for each group the L2 norm of its (grad_scale-scaled) gradient is clipped to max_norm exactly as
 * nn.utils.clip_grad_norm_ does (coef = max_norm / (norm + 1e-6), capped at 1; max_norm <= 0: no clipping), then
 * torch.optim.Adam's update (amsgrad off, weight_decay 0) with the group's lr (host-side schedule) and the given step
 * count (>= 1, for the bias corrections).  Elements outside every group are left untouched (the reference keeps
 * decoder_query_embed out of the optimizer).  grad_scale folds the 1/world_size of a summed data-parallel all-reduce.
 * A group with begin == end is skipped (nothing of it is read or written): a step may be applied in parts -- the groups whose gradients
 * are final early, under the rest of the backward pass; the others at the end -- with the same step count in both calls.
 * norm_ws: [MADE_ADAM_MAX_GROUPS * (1 + MADE_ADAM_NORM_BLOCKS)] f32 device workspace; its first MADE_ADAM_MAX_GROUPS entries
 * return the squared group norms.  The norms are reduced in a fixed order (no atomics), so data-parallel ranks that hold the
 * same all-reduced gradients apply bit-identical updates. */
#define MADE_ADAM_MAX_GROUPS 4
#define MADE_ADAM_NORM_BLOCKS 1024
typedef struct MadeAdamGroup { int64_t begin, end; float lr; float max_norm; } MadeAdamGroup;
int made_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   const MadeAdamGroup* groups, int32_t n_groups, float beta1, float beta2, float eps, int64_t step,
                   float grad_scale, float* norm_ws, void* stream);

/* made_adam_step_device: the same tail with its per-step scalars in DEVICE memory, so that the whole training iteration can sit in
 * one captured hipGraph: `state->step` is incremented by the launch (advance_state != 0: the first call of a step
 * applied in parts; 0: a later part of the same step) and then used for the bias corrections;
 * `state->lr[g]` replaces groups[g].lr (the host-side LambdaLR schedule writes the three floats before it replays the graph). */
typedef struct MadeAdamDeviceState { int64_t step; float lr[MADE_ADAM_MAX_GROUPS]; float bc1, bc2_sqrt; } MadeAdamDeviceState;
int made_adam_step_device(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const MadeAdamGroup* groups, int32_t n_groups, float beta1, float beta2, float eps,
                          MadeAdamDeviceState* state_device, int32_t advance_state, float grad_scale, float* norm_ws, void* stream);

/* made_repack: rebuild the kernel-facing copies of every matrix parameter from the f32 masters in one launch:
 * w (rows x cols, `dtype`; NULL = the kernels read the master itself) and wt = W^T (cols x wt_ld, wt_ld >= rows; NULL = not
 * needed).  `descs_device` is a device array sorted by tile_begin (prefix sum of ceil(rows/64)*ceil(cols/64): one workgroup per
 * 64 x 64 tile). */
typedef struct MadeRepackDesc {
    const float* src; void* w; void* wt;
    int64_t rows, cols, wt_ld, tile_begin;
    int32_t dtype; int32_t _pad;
} MadeRepackDesc;
int made_repack(const MadeRepackDesc* descs_device, int32_t n_desc, int64_t total_tiles, void* stream);

/* ==========================================================================================
 * Evaluation metrics that follow the similarity matrix: computed where the matrix lives.
 * ========================================================================================== */

/* made_recall_ranks: de-duplicated rank of every video's ground-truth music (reference utils/util_test.py:44-70, Recall_metrics
 * with dedup=True).  group_id [Nm] int32 maps every music column to the index of its music id (columns with the same id form a
 * group; built once on the host from the id strings), gt_group [Nv] int32 is the group of each video's ground truth.
 * rank_out[i] = number of other groups whose best similarity in row i exceeds the ground-truth group's best one (0 = retrieved
 * first) -- what walking the descending sort while skipping already-seen ids counts.  Exact ties between different ids are
 * counted as ranked after the ground truth (the reference's order among equal values is that of an unstable sort).
 * top1_out [Nv] (may be NULL): column of the row maximum (lowest index among equal maxima).  n_groups <= 32768. */
int made_recall_ranks(const float* sims, int64_t ld, const int32_t* group_id, const int32_t* gt_group, int64_t Nv, int64_t Nm,
                      int64_t n_groups, int32_t* rank_out, int32_t* top1_out, void* stream);

/* made_span_iou: per sample, the highest-scoring query's span (centre, width) -> (start, end) seconds and its IoU with the
 * ground-truth moment (reference test-MaDe.py:304-313 ranked_preds[0]; music_detr/span_utils.py:119-170 detr_iou /
 * individual_IoU_tensor, discounted = False).  pred_out [N,3] (may be NULL) = (start, end, foreground probability) unclamped. */
int made_span_iou(const float* pred_logits, const float* pred_spans, const float* gt_moment, const float* m_duration,
                  int64_t N, int64_t Q, int32_t fg_label, float max_m_duration, float* iou_out, float* pred_out, void* stream);

/* out[b, :cols_a] = a[b, :], out[b, cols_a:] = c[b, :]; contiguous f32 rows.  The DETR token mask [frame mask ; segment mask]
 * (reference model/model_Uni.py:209 torch.cat); either part may be empty. */
int made_concat_cols(const float* a, int64_t cols_a, const float* c, int64_t cols_c, float* out, int64_t rows, void* stream);

/* ---- the free functions the reference's drivers import (train-MaDe.py:16,20,22); Python mirrors with the
 * reference's names: mgsv_amd/modules/metrics.py, mgsv_amd/modules/loss.py, mgsv_amd/music_detr/span_utils.py ---- */

/* out[a * sa + p * sp] = cos(anchor[a, :], pooled[p, a, :]); anchor f32 [A, D] (row stride lda), pooled [P, A, D] contiguous (f32 or
 * bf16).  reference modules/metrics.py:10-24 sim_matrix_music_pooling (anchor = videos, sa = ld, sp = 1) and :26-41
 * sim_matrix_video_pooling (anchor = tracks, sa = 1, sp = ld). */
int made_pooled_cosine(const float* anchor, int64_t lda, const void* pooled, int32_t pooled_dtype, float* out, int64_t sa, int64_t sp,
                       int64_t A, int64_t P, int64_t D, void* stream);
/* out[i] = x[i] * exp(*logit_scale): the scaled logits of reference modules/loss.py:12-13 (CLIPLoss), :86-88 (InfoNCELoss). */
int made_scale_exp(const float* x, const float* logit_scale, float* out, int64_t n, void* stream);
/* mode 0: (centre, width) -> (start, end) (reference music_detr/span_utils.py:15-24 span_cw_to_se); 1: the inverse (:4-13). [N, 2] f32. */
int made_span_convert(const float* in, float* out, int64_t N, int32_t mode, void* stream);
/* all pairs of spans1 [N, 2] x spans2 [M, 2] (start, end): IoU and union (reference span_utils.py:39-66 temporal_iou), generalised
 * IoU (:86-115), intersection over the second span (:69-83); any output may be NULL.  [N, M] f32 each. */
int made_span_pairwise(const float* spans1, const float* spans2, float* iou, float* uni, float* giou, float* inter_over_2,
                       int64_t N, int64_t M, void* stream);
/* IoU of one predicted (start, end) in seconds per sample with its ground-truth moment (reference span_utils.py:119-170:
 * individual_IoU_tensor; clamp_to_max = 1 adds detr_iou's clamp of the prediction to [0, max_m_duration]). */
int made_span_iou_se(const float* pred_se, const float* gt_moment, const float* m_duration, int64_t N, float max_m_duration,
                     int32_t clamp_to_max, int32_t discounted, float* iou_out, void* stream);

/* ==========================================================================================
 * Grounding: each video's best K tracks and the localization batch of arbitrary (video, track) pairs (mgsv_amd/grounding.py).
 * The reference has no counterpart: it predicts a moment in the ground-truth track only (utils/util_test.py:202-226).
 * ========================================================================================== */

/* made_topk_groups: the best K groups of every row of sims [Nv, Nm] f32 (row stride ld >= Nm).  group_id [Nm] int32 (may be NULL:
 * every column is its own group) maps columns to groups 0 .. n_groups-1, the convention of made_recall_ranks (columns with an id
 * outside that range are ignored).  A group's score is its maximum and its representative column the lowest column attaining it.
 * idx_out [Nv, K] int32 = representative columns, score_out [Nv, K] f32 = scores, in a strict total order: score descending, then
 * column ascending (exact and deterministic); NaN ranks below every number, -0 equals +0.  Positions past the number of non-empty
 * groups hold -1 / -inf.  idx_out[i, 0] equals made_recall_ranks' top1_out[i] (same "lowest index among equal maxima" rule).
 * 1 <= K <= 256; with groups n_groups <= 32768 (one LDS table per row); Nm <= 2^24.  Rows of more than 32768 columns without
 * groups select per block of columns and then over the blocks' candidates: they need `ws` of
 * made_topk_groups_ws_bytes(Nv, Nm, K) bytes (0 otherwise: ws may be NULL). */
int64_t made_topk_groups_ws_bytes(int64_t Nv, int64_t Nm, int64_t K);
int made_topk_groups(const float* sims, int64_t ld, const int32_t* group_id, int64_t Nv, int64_t Nm, int64_t n_groups,
                     int64_t K, int32_t* idx_out, float* score_out, void* ws, int64_t ws_bytes, void* stream);

/* made_eligibility: which columns of a library each video may be grounded in -- per-video constraints on per-column attributes,
 * as a bit matrix for made_topk_groups_masked / made_group_topw_masked.  Column attributes (any may be NULL: that test is off for
 * every row): col_tags [Nm] int64 (64 free bits, compared as unsigned patterns), col_length [Nm] f32 seconds, col_key [Nm] int32
 * (the column's track index, the unit exclusion lists name).  Row constraints: row_all / row_any / row_forbid [Nv] int64 (each may
 * be NULL = 0), row_min / row_max [Nv] f32 (NULL: not tested), ex_start [Nv + 1] int32 and ex_keys [n_ex_keys] int32 a CSR of
 * excluded keys, ascending inside each row (ex_start may be NULL: no lists; ranges are clamped to [0, n_ex_keys]).  Column c
 * (tags T, length L, key t) is eligible for row i iff (T & all_i) == all_i, and any_i == 0 or (T & any_i) != 0, and
 * (T & forbid_i) == 0, and L >= min_i, and L <= max_i (plain f32 comparisons: a NaN length fails a bound that is tested), and t
 * is not in row i's list (binary search; an empty list is not searched).  Outputs, either may be NULL but not both:
 * bits_out [Nv, ld_words] uint32, column c = bit c & 31 of word c >> 5, the bits past Nm of the last word 0, words
 * ceil(Nm / 32) .. ld_words-1 of a row untouched; col_any_out [ceil(Nm / 32)] uint32, the OR over the rows, accumulated with
 * atomicOr: the caller zeroes it.  Refused: a row pattern without col_tags, a bound without col_length, lists without col_key.
 * One thread per column keeps the attributes in registers over a strip of rows; 64 tests are one ballot. */
int made_eligibility(const int64_t* col_tags, const float* col_length, const int32_t* col_key, const int64_t* row_all,
                     const int64_t* row_any, const int64_t* row_forbid, const float* row_min, const float* row_max,
                     const int32_t* ex_start, const int32_t* ex_keys, int64_t n_ex_keys, int64_t Nv, int64_t Nm, uint32_t* bits_out,
                     int64_t ld_words, uint32_t* col_any_out, void* stream);

/* made_topk_groups_masked: made_topk_groups on every row with its ineligible columns removed.  bits [Nv, bits_ld] uint32 is
 * made_eligibility's bits_out (bits_ld >= ceil(Nm / 32)): a column whose bit is clear adds to no group's maximum, represents no
 * group and breaks no tie; a group without an eligible column is absent, and positions past the eligible groups hold -1 / -inf.
 * An eligible -inf or NaN column is still an item.  Everything else -- order, limits, the long-row path and its workspace of
 * made_topk_groups_ws_bytes -- is made_topk_groups'; bits == NULL is that call. */
int made_topk_groups_masked(const float* sims, int64_t ld, const int32_t* group_id, const uint32_t* bits, int64_t bits_ld, int64_t Nv,
                            int64_t Nm, int64_t n_groups, int64_t K, int32_t* idx_out, float* score_out, void* ws, int64_t ws_bytes,
                            void* stream);

/* made_gather_pairs: the localization batch of P (video, track) pairs vi[P], mi[P] (device int32) from per-item tower outputs, in
 * one launch -- what the temporal encoders of a forward over those pairs leave behind.  Video side: frame tokens [Nv, Tv, D]
 * (`dtype`, item stride v_tok_stride elements, rows contiguous), frame mask [Nv, Tv] f32, clip vector [Nv, D] f32; music side
 * the same with Ta segments.  The item strides let the packed music records of the sharded retrieval be read in place.
 * Outputs: frame_out [P, Tv, D] and seg_out [P, Ta, D] (pair strides frame_out_stride / seg_out_stride: both halves of the concat
 * fusion's DETR input, or the CA fusion's two buffers), fmask_out [P, Tv], smask_out [P, Ta], video_out / music_out [P, D] f32.
 * Token rows, token strides and D * element size must be 16-byte aligned (16-byte copies).  A pair with an index outside
 * [0, Nv) x [0, Nm) reads nothing and is written as all padding; its localization outputs are unspecified. */
int made_gather_pairs(const int32_t* vi, const int32_t* mi, int64_t P, int64_t Nv, int64_t Nm,
                      const void* v_tok, int64_t v_tok_stride, const float* v_mask, int64_t v_mask_stride,
                      const float* v_vec, int64_t v_vec_stride,
                      const void* m_tok, int64_t m_tok_stride, const float* m_mask, int64_t m_mask_stride,
                      const float* m_vec, int64_t m_vec_stride, int64_t Tv, int64_t Ta, int64_t D, int32_t dtype,
                      void* frame_out, int64_t frame_out_stride, void* seg_out, int64_t seg_out_stride,
                      float* fmask_out, float* smask_out, float* video_out, float* music_out, void* stream);

/* made_gather_rows: dst[r, :] = src[index[r], :] for r < R, in one launch (a wave per row, 16-byte accesses): the unique AST
 * feature rows of a library spread over the overlapping windows that share them (mgsv_amd/music.py encode_windows).  src [U, C]
 * and dst [R, C] contiguous rows of `dtype` (MADE_F32 or MADE_BF16), index [R] device int32.  An index < 0 or >= U writes a zero
 * row and reads nothing.  C * element size must be a multiple of 16 and both buffers 16-byte aligned. */
int made_gather_rows(const void* src, int64_t U, const int32_t* index, int64_t R, int64_t C, void* dst, int32_t dtype, void* stream);

/* made_group_topw: for every (row i, selected column sel[i, j]) of made_topk_groups' output the best w columns of that column's
 * group in row i of sims [Nv, Nm] f32 (row stride ld >= Nm).  col_group [Nm] int32 is the group of every column (the array
 * made_topk_groups selected with), start [n_groups + 1] / cols [n_cols] int32 the groups' members as a CSR built once on the host:
 * group g holds cols[start[g] .. start[g + 1]); only those members are read, never the row.  idx_out / score_out [Nv, K, w], in
 * made_topk_groups' total order and with its rules: score descending, then column ascending; NaN ranks below every number, -0
 * equals +0 (and is reported as +0).  Position 0 is sel[i, j] itself (the group's representative column).  Positions past the
 * group's size, and every position of a slot with sel < 0, hold -1 / -inf.  Members outside [0, Nm) and CSR ranges outside
 * [0, n_cols] are ignored.  1 <= w <= 16. */
int made_group_topw(const float* sims, int64_t ld, const int32_t* sel, const int32_t* col_group, const int32_t* start,
                    const int32_t* cols, int64_t n_cols, int64_t Nv, int64_t Nm, int64_t n_groups, int64_t K, int64_t w,
                    int32_t* idx_out, float* score_out, void* stream);

/* made_group_topw_masked: made_group_topw with the ineligible members of every group skipped (bits [Nv, bits_ld] uint32 as in
 * made_topk_groups_masked, whose output sel is): a member whose bit is clear fills no slot, so a group left with fewer than w
 * eligible members ends in -1 / -inf.  bits == NULL is made_group_topw. */
int made_group_topw_masked(const float* sims, int64_t ld, const uint32_t* bits, int64_t bits_ld, const int32_t* sel,
                           const int32_t* col_group, const int32_t* start, const int32_t* cols, int64_t n_cols, int64_t Nv, int64_t Nm,
                           int64_t n_groups, int64_t K, int64_t w, int32_t* idx_out, float* score_out, void* stream);

/* made_topk_merge: a running selection merged with the selection of one more chunk of columns, for every row (a selection
 * decomposes over column chunks that hold whole groups: mgsv_amd/library.py, grounding.ground_library).  An entry is a selected
 * group with the w best columns of that group, in made_group_topw's form: col [.., w] int32 (-1: none) and score [.., w] f32
 * (-inf: none), sorted inside the entry; the entry's key is (score[0], col[0]), an entry with col[0] == -1 is empty.  Both lists
 * -- a [Nv, Ka, w] and b [Nv, Kb, w], whose columns are local to the chunk -- are sorted by key in made_topk_groups' total order
 * (score descending through the same order-preserving key, so NaN ranks lowest and -0 equals +0; then column ascending), empty
 * entries last.  out [Nv, K, w] receives the first K entries of the union in that order, payload unchanged except that
 * col_offset is added to every column >= 0 of b (also before b's keys are compared); the rest is filled with -1 / -inf.  No group
 * may occur in both lists and no column twice (nothing is deduplicated); keys that are equal all the same rank in entry order, a
 * before b.  One workgroup per row, no atomics, no workspace; 16-byte accesses when w % 4 == 0 and every buffer is 16-byte
 * aligned.  1 <= K <= 256, 0 <= Ka, Kb <= 256 (an empty list's pointers may be NULL), 1 <= w <= 16, 0 <= col_offset < 2^31; the
 * outputs must not overlap the inputs or each other. */
int made_topk_merge(const int32_t* a_col, const float* a_score, int64_t Ka, const int32_t* b_col, const float* b_score, int64_t Kb,
                    int64_t col_offset, int64_t Nv, int64_t w, int64_t K, int32_t* out_col, float* out_score, void* stream);

/* made_topk_candidates: the selection of a row that is known only at R <= 256 candidate columns (`ground(..., shortlist=R)`).
 * cand_col [Nv, R] int32 (-1 or >= N: no candidate; the columns of a row distinct) and cand_score [Nv, R] f32; col_group [N] int32
 * with ids in [0, n_groups), or NULL (every column its own group).  out_col / out_score [Nv, K, w]: bit for bit what
 * made_topk_groups_masked followed by made_group_topw_masked give on a dense row that holds the candidates' scores at their
 * columns with every other eligibility bit clear -- groups by their best candidate (score descending through the order-preserving
 * key, so NaN ranks lowest and -0 is +0; then column ascending), inside a group its best w candidates in the same order, -1 / -inf
 * past the groups and past a group's candidates.  One workgroup per row, keys in LDS, rank by counting: comparisons only, no
 * float arithmetic, no atomics.  1 <= K <= 256, 1 <= w <= 16; the outputs must not overlap the inputs or each other. */
int made_topk_candidates(const int32_t* cand_col, const float* cand_score, int64_t Nv, int64_t R, const int32_t* col_group, int64_t N,
                         int64_t n_groups, int64_t K, int64_t w, int32_t* out_col, float* out_score, void* stream);

/* made_mmr_select: the greedy re-selection of k results among a pool of P selected groups, for every video independently
 * (`ground(..., diversity= / max_similarity= / pool=)`).  row [Nv, P] int32: the row of `vec` that holds the vector of slot j
 * (< 0 or >= n_rows: the slot is absent), score [Nv, P] f32, vec [n_rows, D] f32 with contiguous rows, 16-byte aligned.  Every
 * present slot keeps m_j, the largest cosine between its vector and the vector of a slot picked so far.  Each of k steps picks,
 * among the present slots neither picked nor dropped, the one with the largest objective score_j - mu * m_j (score_j before the
 * first pick; one f32 fused multiply-add), compared in made_topk_groups' order (descending, -inf below every number, NaN lowest,
 * -0 equals +0), ties to the smaller j; after a pick every m_j is updated and every unpicked slot with m_j > tau is dropped for
 * good; the steps end when no slot is left.  The cosine is a.b / (|a| |b|) in f32 from norms the kernel computes itself; a norm
 * that is zero or not finite gives 0.  pos [Nv, k] int32: the picked slots in pick order, -1 past the last pick; redundancy
 * [Nv, k] f32: m_j of every pick when it was picked, NaN for the first pick and past the last.  With mu = 0 and tau = +inf, and
 * slots in the selection's order, pos is 0, 1, ... over the present slots.  One workgroup per video; the pool's rows are
 * gathered into LDS once when P * D * 4 <= 144 KiB and re-read from `vec` in every step otherwise -- every dot product is summed
 * in one fixed order, so the two forms, any launch and any placement of the rows in `vec` give the same bits.  No atomics, no
 * workspace.  D in {128, 256, 512} (MADE_ERR_UNSUPPORTED otherwise), 1 <= k <= P <= 256, mu finite and >= 0, tau > -1; the
 * outputs must not overlap the inputs or each other. */
int made_mmr_select(const int32_t* row, const float* score, const float* vec, int64_t n_rows, int64_t D, int64_t Nv, int64_t P, int64_t k,
                    float mu, float tau, int32_t* pos, float* redundancy, void* stream);

/* made_cosine_join: the threshold self-join of a vector table, for grouping near-duplicate tracks when a library is built
 * (mgsv_amd/dedup.py near_duplicate_pairs).  vec [N, D] f32 with contiguous rows, 16-byte aligned, N < 2^31; node [N] int32 or NULL.
 * Appends every pair (i, j) with r0 <= i < r1, c0 <= j < c1, i < j, node[i] != node[j] (when node is given) and cos(i, j) >= tau.
 * The cosine is a.b / (|a| |b|) in f32: the table is NOT normalised beforehand, the kernel sums every staged row's squares itself
 * and divides in the epilogue (one f32 product of the two norms, one f32 division); a row whose norm is zero or not finite, or a
 * pair whose product of norms is zero or not finite, joins nothing.  Products run on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32):
 * a dot product is one fmaf chain over the D components in an order that is the same for every tile, range and launch, and a norm
 * is summed in one fixed order per row, so the bits of a pair's cosine depend on the two rows alone -- not on how the table is cut
 * into ranges, on a pair's position in a tile, or on the other rows.  128 x 128 tiles of the rectangle; a tile that lies wholly on
 * or below the diagonal is not computed.  pair_i / pair_j int32 and pair_cos f32 [capacity]; count: one device int64 the call ADDS
 * to (the caller zeroes it): a workgroup prefix-sums its matches and reserves their slots with one atomic add; a match whose slot
 * is >= capacity is counted and not written, so count > capacity tells the caller to repeat the range with larger buffers (slots
 * past min(count, capacity) are left untouched).  The SET of pairs is deterministic; their ORDER in the buffers is not (it is the
 * order in which workgroups reserve).  D in {128, 256, 512} (MADE_ERR_UNSUPPORTED otherwise, and for a rectangle of 2^31 tiles or
 * more); tau in (-1, 1]. */
int made_cosine_join(const float* vec, int64_t N, int64_t D, const int32_t* node, int64_t r0, int64_t r1, int64_t c0, int64_t c1, float tau,
                     int32_t* pair_i, int32_t* pair_j, float* pair_cos, int64_t capacity, int64_t* count, void* stream);

/* made_cosine_topk: the k nearest nodes by cosine of every query row over a vector table ("which tracks are like this track":
 * mgsv_amd/similar.py nearest_columns).  query [Q, D] and vec [N, D] f32 with contiguous rows, 16-byte aligned, read only, NOT
 * normalised beforehand; query may point into vec.  The node of column j is node[j] (int32 [N]), or j itself when node is NULL; a
 * column with node[j] < 0 is ignored (made_topk_groups' convention).  Query i excludes the node query_node[i] (int32 [Q]); a
 * negative value, or a NULL array, excludes nothing -- a row of the table looks itself up with query_node[i] = its own node.  Column
 * j is admissible for query i iff its node is >= 0 and differs from query_node[i], both norms are finite and > 0, the f32 product of
 * the two norms is finite and > 0, and the cosine is not NaN; a query whose norm is zero or not finite has no neighbours.  A node's
 * score is the largest cosine over its admissible columns, its representative the lowest column that attains it.  out_col int32 /
 * out_cos f32 [Q, k]: the best k nodes' representatives and scores in the selection's total order -- score descending through the
 * order-preserving key (so -0 equals +0), then representative column ascending; slots past the nodes present hold -1 / -inf.
 * The cosine is a.b / (|a| |b|) exactly as made_cosine_join forms it (the same fmaf chain over D on v_mfma_f32_32x32x2_f32, the
 * same four-chain sum of squares per row, one f32 product of the norms, one f32 division): a (query row, table row) pair has the
 * bits made_cosine_join gives the same two rows, and they do not depend on Q, N, n_splits, the pair's position in a tile or any
 * other row.  A workgroup takes 128 query rows and walks the 128-column tiles of its column split, keeping every row's sorted list
 * of k entries in LDS; each split writes its lists to ws ([splits, Q, k] of (f32 cos, int32 col)), and a second launch on the same
 * stream merges them by the same order and node rule, so the result is bit-identical for every n_splits.  n_splits = 0: the
 * launcher chooses (enough splits to fill the chip when Q is small); n_splits >= 1 is honoured, clamped to the number of column
 * tiles.  No atomics.  made_cosine_topk_ws_bytes: the bytes ws must hold for a call with these arguments (-1 for arguments the
 * call refuses).  D in {128, 256, 512}, 1 <= k <= 64, N < 2^31, Q < 2^31, ws_bytes >= made_cosine_topk_ws_bytes(...):
 * MADE_ERR_UNSUPPORTED otherwise.  Q = 0 returns MADE_OK and writes nothing; N = 0 fills -1 / -inf.  ws 8-byte aligned; the outputs
 * must not overlap the inputs, the workspace or each other. */
int64_t made_cosine_topk_ws_bytes(int64_t Q, int64_t N, int64_t k, int32_t n_splits);
int made_cosine_topk(const float* query, int64_t Q, const int32_t* query_node, const float* vec, int64_t N, int64_t D, const int32_t* node,
                     int64_t k, int32_t n_splits, int32_t* out_col, float* out_cos, void* ws, int64_t ws_bytes, void* stream);

/* made_cosine_topk_ex: made_cosine_topk under an eligibility mask and with a choice of first-stage kernel.  Everything not named
 * here -- arguments, order, node rule, fill, the bits of a cosine, the workspace layout, the merge launch -- is made_cosine_topk's.
 * bits [Q, bits_ld] uint32 is made_eligibility's matrix with one row per QUERY (bits_ld >= ceil(N / 32), column c = bit c & 31 of
 * word c >> 5; the bits past N of the last word and the words past ceil(N / 32) are not read as columns); NULL: every column is
 * eligible.  "Admissible" gains one clause: the column's bit in the query's row is set.  An ineligible column gives no node its
 * score and represents none; a node without an eligible admissible column is absent; slots past the nodes present hold -1 / -inf.
 * The mask is tested in the first stage only (a template parameter; the unmasked instantiation is made_cosine_topk's code).
 * form: 1 = a workgroup takes 128 query rows (made_cosine_topk's kernel); 2 = a workgroup takes 32 query rows, staged once for its
 * whole walk, and Q > 32 takes several row blocks -- for few queries, where a 128-row tile pays for rows that do not exist; 0 = the
 * launcher chooses.  Both forms run the dot product as the same chain on v_mfma_f32_32x32x2_f32 with the same operand layout, so a
 * (query row, table row) pair has the same bits in both, and the result is bit-identical across forms and splits.
 * made_cosine_topk_ex_ws_bytes: the bytes ws must hold (the forms choose different splits for n_splits = 0); -1 for arguments the
 * call refuses.  form outside 0..2 and ws_bytes below that: MADE_ERR_UNSUPPORTED; bits_ld < ceil(N / 32): MADE_ERR_INVALID_ARG. */
int64_t made_cosine_topk_ex_ws_bytes(int64_t Q, int64_t N, int64_t k, int32_t n_splits, int32_t form);
int made_cosine_topk_ex(const float* query, int64_t Q, const int32_t* query_node, const float* vec, int64_t N, int64_t D,
                        const int32_t* node, const uint32_t* bits, int64_t bits_ld, int64_t k, int32_t n_splits, int32_t form,
                        int32_t* out_col, float* out_cos, void* ws, int64_t ws_bytes, void* stream);

/* made_merge_moments: the moments of P (video, track) entries on the track's own time axis from the moments of the track's w
 * windows, one wave per entry, no atomics.  win_col / win_score [P, w] = made_group_topw's columns (-1: no window) and
 * similarities; cand [P, w, Q, 3] f32 = every query's (start, end, foreground probability) in seconds on its window's axis,
 * unclamped (made_span_iou's pred_out over single-query rows; Q = 1 and use_prob = 0 for the regression head, whose third value
 * is ignored); offset / duration [Nm] f32 = every column's window offset and duration in seconds (duration may be NULL).
 * A candidate's span is clamped to [0, min(max_m_duration, duration[col])], then offset[col] is added (f32).  Total order:
 * window similarity descending, foreground probability descending (skipped when use_prob = 0), column ascending, query
 * ascending; similarities and probabilities compare as in made_topk_groups (NaN lowest, -0 = +0).  Greedy suppression walks
 * that order: a candidate is dropped when its IoU with one kept before it is > nms_iou, with (reference
 * music_detr/span_utils.py:39-66 temporal_iou) inter = max(0, min(e1, e2) - max(s1, s2)), union = (e1 - s1) + (e2 - s2) - inter,
 * iou = union > 0 ? inter / union : 0, f32 with one rounding per operation.  start_out / end_out / conf_out f32 and window_out
 * int32 [P, n]: the first n kept candidates (conf = the probability, NaN when use_prob = 0; window = the candidate's column);
 * slots past the number kept hold NaN / -1.  w * Q <= 256 (MADE_ERR_UNSUPPORTED otherwise); nms_iou >= 0. */
int made_merge_moments(const float* cand, const int32_t* win_col, const float* win_score, const float* offset, const float* duration,
                       int64_t P, int64_t Nm, int64_t w, int64_t Q, int32_t use_prob, float max_m_duration, float nms_iou, int64_t n,
                       float* start_out, float* end_out, float* conf_out, int32_t* window_out, void* stream);

/* ==========================================================================================
 * FP8 token storage of a music library (mgsv_amd/library.py dtype "fp8"; csrc/fp8.hip, csrc/fp8_format.h).  A token row is the D
 * bf16 values of one (column, segment).  It is stored as one int8 exponent e and D bytes:
 *   e       0 for a row of zeros; else the smallest integer with amax * 2^-e <= 448 (amax = max |x| over the row), clamped to
 *           [-120, 120]: with amax = m * 2^ex, m in [0.5, 1), e = ex - 9 if m <= 0.875 and ex - 8 otherwise;
 *   byte    the OCP e4m3fn encoding (not the MI300X fnuz one) of x * 2^-e, round to nearest, ties to even, with subnormals; the
 *           product is exact and at most 448, so neither saturation nor a NaN code arises; -0 keeps its sign;
 *   value   bf16(byte) * 2^e, which is exact in bf16 (a 4-bit significand into 8; 2^-9 * 2^-120 is still a bf16 subnormal).
 * Non-finite tokens have no encoding, and neither have the seven bf16 magnitudes from 248 * 2^120 on (they scale past 248, round
 * to the payload 256 and would widen to 2^128): the callers refuse both before quantising (mgsv_amd/library.py FP8_MAX_TOKEN); a
 * NaN or infinity here would set amax's pattern above every number and give meaningless bytes.  Re-quantising the dequantised row
 * gives the same values, and the same bytes unless the row's scaled maximum rounded down to 224: the smallest exponent is then
 * one less and every byte the code of twice its value.  The reference stores f32 features only.
 * ========================================================================================== */

/* made_fp8_quantize_rows: q [R, D] uint8 and exp [R] int8 of the rows of src [R, D] bf16 (contiguous).  A 16-lane group per row,
 * 16-byte loads, amax by a DPP reduction over the group, the exponent from amax's bits, integer arithmetic on the patterns.  No
 * LDS, no atomics, no workspace.  D in {128, 256, 512} (MADE_ERR_UNSUPPORTED otherwise); src and q 16-byte aligned; the outputs
 * must not overlap the input or each other. */
int made_fp8_quantize_rows(const void* src, int64_t R, int64_t D, uint8_t* q, int8_t* exp, void* stream);

/* made_fp8_dequantize_rows: dst [R * rows_per_index, D] bf16 from q [U, rows_per_index, D] uint8 and exp [U, rows_per_index] int8.
 * index [R] device int32: dst block r = the dequantised block index[r] (rows_per_index = S gathers whole columns of [N, S, D]
 * tokens, every row with its own exponent); an index < 0 or >= U writes a zero block and reads nothing, as made_gather_rows does.
 * index == NULL: blocks 0 .. R - 1 of the given base (R <= U), so a contiguous slice needs no index.  One lane per 16 values: 16
 * payload bytes in, two 16-byte stores out.  No LDS, no atomics, no workspace.  D in {128, 256, 512} (MADE_ERR_UNSUPPORTED
 * otherwise); q and dst 16-byte aligned; dst must not overlap q, exp or index. */
int made_fp8_dequantize_rows(const uint8_t* q, const int8_t* exp, int64_t U, const int32_t* index, int64_t R, int64_t rows_per_index,
                             int64_t D, void* dst, void* stream);

/* ==========================================================================================
 * Frames: decoded video frames -> the input of the CLIP ViT-B/32 visual tower (mgsv_amd/frames.py).  The reference extracts its
 * frame features with OpenAI's clip package (model/model_Base.py:286-289,406-450) after torchvision preprocessing
 * (dataloaders/dataloader_MGSV_EC_rawdata.py:16-25); the tower itself runs on made_linear / made_layernorm / made_attention.
 * ========================================================================================== */

#define MADE_FRAMES_MAX (1 << 20)      /* most frames one made_frames_preprocess call takes */

/* One frame of the packed input.  The coefficient block at coef[coef ..] holds 224 rows of (first input column, tap count, kh
 * int32 taps) for the crop's output columns, then 224 rows of (first input row, tap count, kv taps) for its output rows: PIL's
 * bicubic taps in 22-bit fixed point, computed on the host (mgsv_amd/frames.py pil_taps) with the centre crop folded in.  A pass
 * PIL skips (that side is already 224) is one tap of 1 << 22 at the cropped position. */
typedef struct MadeFrameDesc {
    int64_t offset;        /* byte offset of the frame's first pixel in `frames` (RGB, 3 bytes per pixel, rows of 3 W bytes) */
    int64_t coef;          /* index (int32 elements) of the frame's coefficient block */
    int32_t H, W;          /* input rows and columns */
    int32_t kh, kv;        /* taps per row of the horizontal / vertical block, 1 .. 255 */
} MadeFrameDesc;

/* made_frames_preprocess: torchvision Resize(224, BICUBIC) + CenterCrop(224) + ToTensor + Normalize(CLIP mean, std) of n_frames
 * frames of any and mixed sizes, in one launch (a workgroup per frame and band of 16 output rows; the horizontal pass through
 * LDS, integer arithmetic as PIL's, so the crop is bit-exact).  desc [n_frames] and coef [n_coef] are device arrays.  Writes the
 * 49 patch rows of every frame: patches[(f * 49 + p) * ld_patch + c * 1024 + y * 32 + x] = (u / 255 - mean_c) / std_c (f32, one
 * rounding per operation) for pixel (y, x) of patch p = 7 * patch row + patch column, channel c -- the A operand of conv1
 * (conv1.weight.reshape(768, 3072)); patch_dtype MADE_F32 or MADE_BF16 (rounded from that f32 value).  crop_out (may be NULL):
 * the uint8 crop [n_frames, 224, 224, 3].  Reads stay inside each frame and block; a descriptor that does not fit frames_bytes /
 * n_coef gives NaN patch rows and a zero crop. */
int made_frames_preprocess(const uint8_t* frames, int64_t frames_bytes, const MadeFrameDesc* desc, int64_t n_frames,
                           const int32_t* coef, int64_t n_coef, void* patches, int32_t patch_dtype, int64_t ld_patch,
                           uint8_t* crop_out, void* stream);

/* ==========================================================================================
 * Audio: decoded PCM -> the input of the AST tower (mgsv_amd/music.py).  The reference computes its AST segment features from raw
 * audio (dataloaders/dataloader_MGSV_EC_rawdata.py:95-158 get_ast_rawaudio, model/model_Base.py:273-282,472-499): torchaudio's
 * resample to 16 kHz, sliding segments, Kaldi fbank, then a DeiT-base AST; the tower itself runs on made_linear / made_layernorm /
 * made_attention.
 * ========================================================================================== */

#define MADE_AUDIO_TRACKS_MAX (1 << 16)   /* most tracks one made_audio_resample call takes */
#define MADE_AUDIO_SEGS_MAX (1 << 20)     /* most segments one made_audio_fbank / made_ast_patches call takes */
#define MADE_RESAMPLE_TILE 1024           /* output samples per workgroup of made_audio_resample */
#define MADE_RESAMPLE_SLAB 12288          /* most input samples a workgroup stages: ((TILE - 1) / m + 1) * o + taps must fit */
#define MADE_AUDIO_ROWS 1024              /* spectrogram rows (AST's input_tdim) */
#define MADE_AUDIO_MELS 128               /* mel bins */

/* One track of made_audio_resample: torchaudio.functional.resample's polyphase FIR (sinc_interp_hann, lowpass_filter_width 6,
 * rolloff 0.99) from o to m (the rates divided by their gcd) with the taps computed on the host (mgsv_amd/music.py resample_taps).
 * The tap block at taps[taps ..] is k-major: K[p, k] at taps[taps + k * m + p] for k < 2 width + o, p < m.  o == m == 1 is a copy. */
typedef struct MadeResampleDesc {
    int64_t offset;        /* index (floats) of the track's first sample in `pcm` (one channel) */
    int64_t n;             /* input samples */
    int64_t taps;          /* index (floats) of the track's tap block (unused for a copy) */
    int32_t o, m;          /* reduced input / output rates */
    int32_t width;         /* the FIR's half width: `width` zeros in front of the input, width + o behind */
    int32_t _pad;
} MadeResampleDesc;

/* made_audio_resample: n_tracks tracks of mixed rates in one launch (a workgroup per track and tile of MADE_RESAMPLE_TILE outputs; the
 * input slab the tile reads is staged in LDS, the taps are read through the cache).  out [n_tracks, out_len] f32: row t holds
 * y[j] = sum_k K[p, k] x~[b o + k] (j = b m + p, f32 accumulation in k order) for j < min(ceil(m n / o), out_len) and 0 after, x~
 * being the input with `width` zeros in front.  A copy writes x[j] unchanged for j < min(n, out_len).  A descriptor that does not fit
 * pcm_len / n_taps, or whose slab exceeds MADE_RESAMPLE_SLAB, gives a NaN row. */
int made_audio_resample(const float* pcm, int64_t pcm_len, const MadeResampleDesc* desc, int64_t n_tracks, const float* taps,
                        int64_t n_taps, float* out, int64_t out_len, void* stream);

/* One segment of made_audio_fbank: samples pcm[first .. first + count) of the 16 kHz buffer. */
typedef struct MadeAudioSegDesc {
    int64_t first;
    int64_t count;
} MadeAudioSegDesc;

/* made_audio_fbank: torchaudio.compliance.kaldi.fbank(seg, htk_compat=True, sample_frequency=16000, use_energy=False,
 * window_type='hanning', num_mel_bins=128, dither=0.0, frame_shift=10) of n_segs segments, padded / truncated to 1024 rows and
 * normalised as (x + 4.2677393) / 9.1379948 (f32), the reference's `audio` tensor.  A workgroup per segment and tile of 16 rows; each
 * wave takes one 400-sample frame (every 160 samples; n_frames = 1 + (count - 400) / 160, 0 when count < 400): mean removal,
 * pre-emphasis 0.97, the window, a 512-point radix-2 FFT in LDS (f32), |X|^2, the mel filters, log(max(e, 2^-23)) (the floor's log
 * is a constant).  window [400] f32, twiddle [512] f32 (cos(2 pi k / 512) for k < 256, then sin), mel [128, mel_ld] f32 rows of
 * (first bin, bin count, weights), all computed on the host in float64 (mgsv_amd/music.py fbank_tables).  Rows >= n_frames hold the
 * padded value 4.2677393f / 9.1379948f.  spec [n_segs, 1024, 128] f32.  A segment that does not fit pcm_len gives NaN rows. */
int made_audio_fbank(const float* pcm, int64_t pcm_len, const MadeAudioSegDesc* segs, int64_t n_segs, const float* window,
                     const float* twiddle, const float* mel, int32_t mel_ld, float* spec, void* stream);

/* made_ast_patches: the patch rows of AST's Conv2d(1 -> 768, 16 x 16, stride 10) over the transposed spectrogram, as a GEMM operand
 * (patch_embed.proj.weight.reshape(768, 256)): patches[(s * 1212 + 101 fi + ti) * ld_patch + 16 k + l] = spec[s, 10 ti + l, 10 fi + k]
 * for fi < 12, ti < 101, k, l < 16.  spec [n_segs, 1024, 128] f32; patch_dtype MADE_F32 or MADE_BF16 (rounded). */
int made_ast_patches(const float* spec, int64_t n_segs, void* patches, int32_t patch_dtype, int64_t ld_patch, void* stream);

/* ==========================================================================================
 * Onsets and fitted moments (mgsv_amd/onsets.py, mgsv_amd/grounding.py fit_grounding; csrc/onsets.hip, csrc/fit.hip).  A track's
 * attacks are found once, from made_audio_fbank's spectrogram of the whole track: block j of a track is the "segment" first =
 * j * 1024 * 160, count = min(n16 - first, 1023 * 160 + 400), whose 1024 rows are the track's frames 1024 j .. 1024 j + 1023 (the
 * fbank removes the mean per frame, so a frame does not depend on the segmentation).  A track of n16 samples has F = 1 + (n16 - 400)
 * / 160 frames of 10 ms (0 below 400 samples); rows past F hold the pad value and are never read as signal.  The reference has no
 * counterpart: it returns the regressed span as it is.
 * ========================================================================================== */

/* made_onset_strength: the spectral flux of N tracks.  logmel [N, F_ld, 128] f32 (16-byte aligned), n_frames [N] device int32, env
 * [N, env_ld] f32:
 *     env[t, f] = (1 / 128) * sum_b max(0, x[t, f, b] - x[t, f - lag, b])     for lag <= f < n_frames[t]
 *     env[t, f] = 0                                                           for every other f < env_ld
 * in the spectrogram's normalised units.  32 lanes per frame, two 16-byte loads per lane, the four differences of a lane added as
 * (d0 + d1) + (d2 + d3) and the lanes by a fixed DPP tree: a frame's bits depend on its own 2 * 128 values only -- not on N, the
 * track's place in the batch, F_ld or env_ld.  Rows >= n_frames[t] of logmel are not read.  No LDS, no atomics, no workspace.  A
 * track with n_frames[t] > F_ld (or < 0) gets a NaN row.  lag in [1, 8]; N == 0 is a no-op.  Refused: negative sizes, lag out of
 * range, null pointers (logmel may be NULL when F_ld == 0, env when env_ld == 0), a logmel that is not 16-byte aligned. */
int made_onset_strength(const float* logmel, int64_t F_ld, const int32_t* n_frames, int64_t N, int32_t lag, float* env, int64_t env_ld,
                        void* stream);

/* made_onset_peaks: the onsets of N tracks from their envelopes env [N, env_ld] f32.  Frame f < n_frames[t] is an onset iff
 *   1. env[f] > 0;
 *   2. env[f] > env[g] for g in [f - w_max, f) and env[f] >= env[g] for g in (f, f + w_max], the windows clipped to [0, n_frames):
 *      exact f32 comparisons; of equal neighbouring values the earlier wins;
 *   3. env[f] >= s / n + delta, s the f32 sum in ascending frame order of env over [f - w_avg, f + w_avg] clipped to [0, n_frames)
 *      and n the number of frames in it.
 * count[t] int32 = the number of onsets; time[t * cap + i] f32, i < count[t] = the onsets ascending as (float)f * 0.01f seconds:
 * the start of the first frame that shows the rise, at or before the attack.  Entries from count[t] on are not written.  Rule 2
 * keeps two onsets w_max + 1 frames apart, so cap >= ceil(env_ld / (w_max + 1)) never overflows (a smaller cap is refused).  One
 * workgroup per track walks tiles of 1024 frames with a 128-frame halo in LDS; the compaction is ordered (ballot, prefix popcount,
 * a running offset): no atomics, no workspace, and a track's list does not depend on the other tracks.  A track with n_frames[t]
 * > env_ld (or < 0) gets count -1 and no entries.  w_max in [1, 32], w_avg in [1, 128], delta finite and >= 0; N == 0 is a no-op.
 * Refused: those ranges, negative sizes, null pointers (env may be NULL when env_ld == 0, time when cap == 0). */
int made_onset_peaks(const float* env, int64_t env_ld, const int32_t* n_frames, int64_t N, int32_t w_max, int32_t w_avg, float delta,
                     int64_t cap, float* time, int32_t* count, void* stream);

/* made_fit_moments: E moments fitted to a wanted length, their track and its onsets; one thread per entry, every step one rounded
 * f32 operation (no contraction), max(a, b) = a > b ? a : b and min(a, b) = a < b ? a : b.  start / end [E] f32 seconds on the
 * track's axis, track [E] int32 (-1: none), want [E] f32 (NaN: keep the moment's own length), tlen [n_tracks] f32, onset_start
 * [n_tracks + 1] int64 and onset_time [n_onsets] f32 the tracks' onsets as a CSR, strictly ascending inside a track, tol f32.
 *   1. track outside [0, n_tracks), or start, end or tlen[track] NaN: out_start = out_end = shift = NaN, onset = -1.
 *   2. T = tlen[track]; len = want if it is not NaN, else end - start; len = min(max(len, 0), T).
 *   3. c = 0.5f * (start + end); s1 = c - 0.5f * len; s1 = min(max(s1, 0), T - len).
 *   4. With tol > 0: among the track's onsets o with fabsf(o - s1) <= tol and o <= T - len the one with the smallest fabsf(o - s1),
 *      of two equal ones the earlier (a binary search for the first o >= s1, then it and the one before): s2 = o and onset = its
 *      index inside the track; without one, or with tol == 0, s2 = s1 and onset = -1.
 *   5. out_start = s2, out_end = s2 + len, shift = s2 - start.
 * onset_start / onset_time may be NULL with tol == 0 (length fitting alone).  E == 0 is a no-op.  Refused: tol negative or not
 * finite, E or n_tracks negative or >= 2^31, n_onsets negative, null required pointers, tol > 0 without the table. */
int made_fit_moments(const float* start, const float* end, const int32_t* track, const float* want, int64_t E, const float* tlen,
                     int64_t n_tracks, const int64_t* onset_start, const float* onset_time, int64_t n_onsets, float tol, float* out_start,
                     float* out_end, float* shift, int32_t* onset, void* stream);

/* ---- Cut sync (mgsv_amd/grounding.py fit_grounding with Fit.cuts; csrc/sync.hip) -----------------------------------------------
 * made_sync_moments: made_fit_moments for a video that is assembled from clips -- the start is chosen so that the video's cuts
 * land on the track's onsets, and how well they do is reported.  start, end, track, want, tlen and the onset CSR are
 * made_fit_moments' arguments.  video [E] int32 is the entry's video (negative or >= n_videos: no cuts); cut_start [n_videos + 1]
 * int64 and cut_time [n_cuts] f32 are the videos' cuts as a CSR, seconds from the video's beginning, ascending inside a video.
 * snap f32: how far the start may move from where made_fit_moments would put it without snapping; cut_tol f32: how near an onset a
 * cut must fall to count.  Every step is one rounded f32 operation (no contraction), comparisons written out.
 *   1. len, c, last = T - len and s1 exactly as made_fit_moments' steps 1 - 3; s1 is the unsnapped start.  A NaN start, end or
 *      tlen[track], or a track outside [0, n_tracks): out_start = out_end = shift = sync = NaN, onset = anchor = hits = -1.
 *   2. Anchors: A = [0] followed by the video's cuts c with c > 0 && c < len, in order (the one predicate drops a NaN, a cut that
 *      is not positive and a cut outside the fitted moment).  At most the first 63 cuts of a row are read, so |A| <= 64: a safety
 *      limit, not a feature -- the Python layer refuses a longer row.
 *   3. Candidates: s1 itself, always; and for every anchor a = A[j] (j ascending) and every onset o of the track (index i
 *      ascending) s = o - a when fabsf(s - s1) <= snap && s >= 0 && s <= last, all three on the rounded s.  For a fixed a each
 *      test is monotone in o: the admitted onsets are one contiguous range, found by binary searches with the same predicate.
 *   4. Score of a start s: sync(s) = the f32 sum, in the order of A from 0, of t(d_a); p = s + a, d_a the smaller of p - o_prev and
 *      o_next - p for the onsets either side of p (o_next the first onset >= p by binary search, o_prev the one before it; a
 *      side that does not exist is skipped); t(d) = d <= cut_tol ? 1 - d / cut_tol : 0; hits(s) = the number of anchors with d_a <=
 *      cut_tol.  A track without onsets scores 0 and 0.
 *   5. Choice, a strict order: larger sync, then smaller fabsf(s - s1), then smaller s, then smaller j, then smaller i; the s1
 *      candidate carries j = +infinity.  So when s1 coincides with an (o, a) candidate the snapped description is reported, and
 *      otherwise a start that need not move does not move.
 *   6. out_start = s, out_end = s + len, shift = s - start; onset = i inside the track's list and anchor = j (both -1 when the
 *      s1 candidate won; anchor 0: the start sits on the onset, j >= 1: anchor j, a cut, does); sync f32, hits int32.
 * For a video without usable cuts (A = [0]) and an onset table without negative times, out_start, out_end, shift and onset are
 * made_fit_moments(tol = snap)'s bit for bit.  One wave per entry, four entries per 256-thread workgroup; anchors and the candidate
 * prefix in LDS, a butterfly reduction with the comparator of step 5 (strict, so the result does not depend on the reduction's
 * shape); no atomics, no workspace, no scratch.  E == 0 is a no-op.  onset_time may be NULL with n_onsets == 0, cut_time with
 * n_cuts == 0, cut_start with n_videos == 0, onset_start and tlen with n_tracks == 0.  Refused: E, n_tracks or n_videos outside
 * [0, 2^31), negative n_onsets or n_cuts, snap or cut_tol not finite or not > 0, null required pointers. */
int made_sync_moments(const float* start, const float* end, const int32_t* track, const int32_t* video, const float* want, int64_t E,
                      const float* tlen, int64_t n_tracks, const int64_t* onset_start, const float* onset_time, int64_t n_onsets,
                      const int64_t* cut_start, const float* cut_time, int64_t n_videos, int64_t n_cuts, float snap, float cut_tol,
                      float* out_start, float* out_end, float* shift, int32_t* onset, int32_t* anchor, float* sync, int32_t* hits,
                      void* stream);

/* ---- Beat grids (mgsv_amd/beats.py; csrc/beats.hip) -----------------------------------------------------------------------------
 * One tempo and the beat times of a track, from made_onset_strength's envelope (frames of 10 ms).  A beat list is "a CSR of
 * ascending times per track": made_fit_moments and made_sync_moments take it where they take the onsets.
 *
 * made_tempo_autocorr: env [N, env_ld] f32 as made_onset_strength writes it, n_frames [N] device int32, 1 <= lag_min <= lag_max
 * <= 256, n_lags = lag_max - lag_min + 1, weight [n_lags] device f32 (the tempo prior of the lags lag_min + j, rounded once by the
 * host).  Outputs ac [N, n_lags + 1] f32, scale [N] f32, period [N] int32.  Per track t with nf = n_frames[t] and e = env[t]:
 *   1. m = (the f32 sum of e[0 .. nf)) / (float)nf; x[f] = e[f] - m.
 *   2. ac[t, 0] = sum_f x[f]^2.
 *   3. ac[t, 1 + j] = sum_{f = l}^{nf - 1} x[f] * x[f - l] for l = lag_min + j (an empty sum, 0, when nf <= l).
 *   4. scale[t] = 1.f / sqrtf(ac[t, 0] / (float)nf): the envelope's inverse standard deviation (three rounded operations).
 *   5. score[j] = (ac[t, 1 + j] / (float)(nf - l)) * weight[j]: two rounded operations.
 *   6. period[t] = the lag of the largest score, of equal scores the smaller lag.
 * A track has no tempo -- period = -1, scale = NaN -- when nf <= lag_max, when ac[t, 0] is not > 0 (a NaN included), or when no
 * score is > 0 (ac is still written).  A track with nf < 0 or nf > env_ld gets that and a NaN ac row; nothing of it is read.
 * Summation order (f32, no contraction; it depends on nf alone, not on N or the track's place in the batch).  The mean: 1024
 * chains, chain i adds e[i], e[i + 1024], ... ascending (ceil(nf / 1024) terms); the 64 chains of a wave meet in a tree of depth 6,
 * the sixteen waves' totals are added in order (15 more additions).  A sum of steps 2 - 3: the track is cut into tiles of 1024
 * frames; inside a tile 64 chains, chain i adding the products of the frames f0 + i, f0 + i + 64, ... ascending (16 terms; a frame
 * outside [l, nf) adds +0), a tree of depth 6 over the chains, and the tiles' totals added ascending (ceil(nf / 1024) terms): a
 * product passes through at most 16 + 6 + ceil(nf / 1024) additions.  One workgroup of sixteen waves per track; the tile and the
 * 256 frames before it are staged in LDS as x; the waves split the lags; no atomics, no workspace.  N == 0 is a no-op.  Refused:
 * negative sizes, lags outside the range, null pointers (env may be NULL when env_ld == 0), N >= 2^31, env_ld >= 2^24. */
int made_tempo_autocorr(const float* env, int64_t env_ld, const int32_t* n_frames, int64_t N, int32_t lag_min, int32_t lag_max,
                        const float* weight, float* ac, float* scale, int32_t* period, void* stream);

/* made_beat_track: the beats of N tracks by Ellis's dynamic programme, every step one rounded f32 operation (no contraction).  env,
 * n_frames as above; period [N] int32 and scale [N] f32 as made_tempo_autocorr writes them (any source will do); alpha f32 the
 * tightness; outputs time [N, cap] f32, count [N] int32, cum [N, env_ld] f32, back [N, env_ld] int32.  With P = period[t]:
 *   1. dlo = (P + 1) / 2 (integer division), dhi = 2 P.
 *   2. pen[d] = -alpha * ((float)((d - P) * (d - P)) / (float)(d * P)) for d in [dlo, dhi]: the integers are exact, a division and
 *      a product.  It is 0 at d = P, symmetric under d -> P^2 / d, and close to alpha * ln^2(d / P).
 *   3. local[f] = e[f] * scale[t].
 *   4. For f = 0 .. nf - 1: best = the largest cum[f - d] + pen[d] over d in [dlo, dhi] with f - d >= 0, of equal sums the smaller
 *      d (a NaN sum is no candidate).  If there is a candidate and best > 0: cum[f] = local[f] + best, back[f] = f - d.  Otherwise
 *      cum[f] = local[f], back[f] = -1: starting afresh is always allowed and costs nothing.
 *   5. End frame = the argmax of cum over [max(0, nf - dhi), nf), of equal values the earlier frame (NaN is no candidate).
 *   6. The beats are the chain end, back[end], back[back[end]], ... down to -1, written ascending as (float)f * 0.01f seconds to
 *      time[t * cap + i]; count[t] = their number (0 when nf == 0).  Entries from count[t] on are not written; of a cum / back row
 *      only [0, nf) is.
 * Two beats are dlo frames apart or more, so a track has at most ceil(nf / dlo) beats.  Per track: period[t] == -1 gives count 0;
 * nf outside [0, env_ld], a period outside {-1} and [2, 256], a scale that is not finite, or cap < ceil(nf / dlo) give count -1;
 * in both cases nothing else of the track is written.  The host cannot see the periods: it refuses a cap < ceil(env_ld / 128),
 * which no period makes safe; cap = env_ld / dlo_min + 1 for the smallest dlo the caller allows never overflows.
 * One workgroup of sixteen waves per track.  Frame f reads frames <= f - dlo only, so the dlo frames f .. f + dlo - 1 are
 * independent: that is the unit between two barriers.  A row of 16 lanes takes a frame (four frames a wave), its lanes the
 * candidates d = dlo + lane, + 16, ... (at most 25), and two DPP maximum reductions over the row give the argmax under the strict
 * order of step 4, which therefore does not depend on the reduction's shape.  The trailing 1024 values of cum, the envelope two
 * tiles of 1024 frames ahead and the pen table live in LDS; cum and back in global memory are written, and back is read only by
 * the backtrace: one thread's walk into LDS (the first 4096 beats; the rest by a second walk), written out in ascending order by
 * all threads.  No atomics, no workspace.
 * alpha finite and >= 0; N == 0 is a no-op.  Refused: negative sizes, such an alpha or cap, null pointers (env, cum and back may be
 * NULL when env_ld == 0, time when cap == 0), N >= 2^31, env_ld >= 2^24. */
int made_beat_track(const float* env, int64_t env_ld, const int32_t* n_frames, const int32_t* period, const float* scale, int64_t N,
                    float alpha, int64_t cap, float* time, int32_t* count, float* cum, int32_t* back, void* stream);

/* ---- Bar grids (mgsv_amd/bars.py; csrc/bars.hip) --------------------------------------------------------------------------------
 * The metre, the phase and the downbeats of a track, from its log-mel spectrogram and its beat list.  A downbeat list is again "a
 * CSR of ascending times per track": made_fit_moments and made_sync_moments take it where they take the onsets or the beats.
 *
 * made_beat_sync_mean: the mean spectrum of every beat's interval.  spec [N, spec_ld, 128] f32 (made_audio_fbank's rows, one track
 * after the other), n_frames [N] device int32, time [N, cap] f32 and count [N] int32 as made_beat_track writes them (any ascending
 * list will do), beat_start [N + 1] device int64 the exclusive prefix of the counts; output B [total_beats, 128] f32, track t's
 * beat k in row beat_start[t] + k.  Per track with n = count[t], nf = n_frames[t]:
 *   1. b_k = (int)(time_k * 100.0f + 0.5f), two rounded operations, kept inside [0, nf] (a NaN or negative time gives 0, a frame
 *      >= nf gives nf).  For every f < 2^20 this inverts made_beat_track's (float)f * 0.01f exactly.
 *   2. The interval of beat k is [b_k, e_k): e_k = b_{k+1} for k < n - 1; e_{n-1} = b_{n-1} + (b_{n-1} - b_{n-2}) for n >= 2 and
 *      b_0 + 1 for n == 1, clipped to nf.  Its length is L = e_k - b_k.
 *   3. B[k, m] = (the f32 sum of spec[f, m] over b_k <= f < e_k) / (float)L; a row of +0 when L <= 0 (an empty interval, or a list
 *      that does not ascend).
 * Summation order (f32; it depends on L alone, not on N, k, cap or the track's place in the batch): a bin has 8 chains, chain c
 * adding the frames b_k + c, b_k + c + 8, ... ascending from +0 (ceil((L - c) / 8) terms), and the chains meet in the tree
 * ((c0 + c2) + (c4 + c6)) + ((c1 + c3) + (c5 + c7)).  A value passes through at most ceil(L / 8) + 2 rounded additions (the first
 * term of a chain is added to +0, which is exact) and the division: depth = ceil(L / 8) + 3, and |B - exact| <= depth * 2^-24 *
 * sum|x| / L to first order.
 * A track with count <= 0 or count > cap, nf outside [0, spec_ld], or beat_start[t + 1] - beat_start[t] != count[t] (or rows
 * outside [0, total_beats)) writes nothing.  A wave takes a beat: lanes own four bins with one 16-byte load per frame, the two
 * halves of the wave the even and the odd frames, four loads in flight per lane; an interval of any length is walked by its one
 * wave.  The spectrogram is read once; no atomics, no workspace, no scratch.  N == 0 is a no-op.  Refused: negative sizes, spec_ld
 * >= 2^20 (step 1), N or total_beats >= 2^31, null pointers (spec may be NULL when spec_ld == 0, time when cap == 0, B when
 * total_beats == 0). */
int made_beat_sync_mean(const float* spec, int64_t spec_ld, const int32_t* n_frames, const float* time, int64_t cap, const int32_t* count,
                        const int64_t* beat_start, int64_t N, int64_t total_beats, float* B, void* stream);

/* made_bar_pick: metre, phase and downbeats of N tracks.  B, beat_start, time / cap as above (track t has n = beat_start[t + 1] -
 * beat_start[t] beats); metre_mask: bit m set for every metre m that is tried, a non-empty set of integers in [2, 8] passed by
 * value; low_bins in [0, 128], low_weight f32 >= 0, min_bars >= 1, min_strength f32 >= 0.  Outputs evidence [total_beats] f32,
 * metre / phase [N] int32, strength [N] f32, down_time [N, cap_d] f32, down_count [N] int32.  Every step below is one rounded f32
 * operation unless it says otherwise (no contraction).  Per track:
 *   1. e[0] = 0; for k >= 1, e[k] = (1/128) * sum_m w_m * max(0, B[k, m] - B[k-1, m]), w_m = 1.f + low_weight for m < low_bins and
 *      1 otherwise (a NaN difference adds 0): the energy that arrives at beat k against the beat before it.  The 128 terms meet as
 *      t[l] + t[l + 64] for l = 0 .. 63, then in a tree of depth 6 over l (pairs l ^ 1, l ^ 2, rotations by 4 and 8 inside each 16,
 *      then the four sixteens), then the exact product with 2^-7: a term passes through a subtraction, a product and 7 additions
 *      (with w_m's own rounding: depth 10).
 *   2. tot = e[1] + e[2] + ... + e[n - 1], one chain, ascending, from +0.  mean_all = tot / (float)(n - 1).
 *   3. For every metre m of the set and every phase phi in [0, m): the members are the beats k >= 1 with k % m == phi, cnt their
 *      number, s their sum (one chain, ascending, from +0); score = s / (float)cnt - mean_all.  (m, phi) is a candidate iff cnt >=
 *      min_bars and the score is not NaN.
 *   4. The pick is the candidate with the largest score, of equal scores the smaller m, then the smaller phi.  strength = score /
 *      mean_all.
 *   5. No metre -- metre = 0, phase = -1, strength = NaN, down_count = 0 -- when n < 2, when there is no candidate, when mean_all is
 *      not > 0, or when strength < min_strength or is NaN.
 *   6. Otherwise metre = m, phase = phi, and the downbeats are the beats phi, phi + m, ... < n (beat 0 when phi == 0), written
 *      ascending with the beats' own f32 times to down_time[t * cap_d + i]; down_count = their number, or -1 (and no time written)
 *      when it exceeds cap_d.  Entries from down_count on are not written.
 * A track whose list does not fit its arrays (n < 0, n > cap, rows outside [0, total_beats)) gets metre 0, phase -1, strength NaN,
 * down_count -1 and no evidence.  One workgroup of sixteen waves per track: waves take the beats of step 1 and keep e in LDS for
 * n <= 4096 (a longer track reads it back from `evidence` after a fence and a barrier); one thread per chain walks steps 2 - 3 (at
 * most 36 chains); one thread walks the candidates in (m, phi) order with a strict >, so the pick does not depend on any
 * reduction's shape.  No atomics, no workspace, no scratch.  N == 0 is a no-op.  Refused: negative sizes, a metre_mask that is 0
 * or has a bit outside 2 .. 8, low_bins outside [0, 128], low_weight or min_strength negative or not finite, min_bars < 1, cap_d <
 * ceil(cap / 2) (every second beat may be a downbeat), N or total_beats >= 2^31, null pointers (B and evidence may be NULL when
 * total_beats == 0, time when cap == 0, down_time when cap_d == 0). */
int made_bar_pick(const float* B, const int64_t* beat_start, const float* time, int64_t cap, int64_t N, int64_t total_beats,
                  int32_t metre_mask, int32_t low_bins, float low_weight, int32_t min_bars, float min_strength, float* evidence,
                  int32_t* metre, int32_t* phase, float* strength, float* down_time, int64_t cap_d, int32_t* down_count, void* stream);

/* ---- Section boundaries (mgsv_amd/sections.py; csrc/sections.hip) ---------------------------------------------------------------
 * Where the timbre of a track changes, from its beat-synchronous spectra B (made_beat_sync_mean).  A boundary list is again "a CSR of
 * ascending times per track": made_fit_moments and made_sync_moments take it where they take the onsets, the beats or the downbeats.
 * The rule is Foote's novelty -- a checkerboard kernel slid along the diagonal of the cosine self-similarity matrix -- with the
 * rank-one kernel C(i, j) = c_i c_j (a sign pattern times a separable taper), for which sum_ij c_i c_j <u_{k+i}, u_{k+j}> is the
 * squared distance between the weighted sum of the L beats after beat k and that of the L beats before it: no n x n matrix is
 * formed and B is read once.  The reference has no counterpart.
 *
 * made_section_novelty.  B [total, 128] f32, beat_start [N + 1] device int64 (track t has the rows r0 = beat_start[t] .. r1 =
 * beat_start[t + 1], n = r1 - r0 beats), weights [L] device f32 (ops.section_weights: the taper, computed on the host, so no device
 * expf enters the contract), 1 <= L <= 64; output novelty [total] f32.  Every step is one rounded f32 operation (no contraction).
 * Per track:
 *   1. For each beat k: m = (the sum of the row's 128 bins) * 2^-7, x = B[k] - m, q = sum x * x, and u_k = x / sqrt(q) (a correctly
 *      rounded square root, then one division per bin) when q > 0 and q is finite, a row of +0 otherwise (a silent or constant beat,
 *      a row holding a NaN or an infinity).
 *   2. For L <= k <= n - L: a = sum_{i = 0}^{L - 1} weights[i] * u_{k + i}, b = sum_{i = 0}^{L - 1} weights[i] * u_{k - 1 - i} (per
 *      bin), novelty[k] = sum over the 128 bins of (a - b) * (a - b).  Every other beat of the track gets exactly +0; with n < 2 L
 *      the whole track is zeros.
 * Summation orders (they depend on L and on nothing else: not on k, n, N, total, the track's place in the batch or the tile of the
 * launch a beat falls in, so a track's novelty has the same bits alone and in any batch).  A 128-term sum (m, q, novelty) meets as
 * t[l] + t[l + 64] for l = 0 .. 63, then in the tree of depth 6 over l that made_bar_pick's step 1 states: 7 rounded additions on a
 * term's way.  An L-term sum (a, b) is one chain per bin, i ascending from +0, each product rounded before it is added: a term
 * passes through its product and at most L additions (the first one, to +0, is exact).  Error, to first order with eps = 2^-24:
 * |m - exact| <= 7 eps mean|B[k]|, so the computed x is off by dx with |dx|_2 <= sqrt(128) 7 eps mean|B[k]| + eps |x|_2, and
 * |u_k - exact|_2 <= e_k = 2 |dx|_2 / |x|_2 + 6 eps (the squares, the 7 additions, the root and the division scale a unit vector);
 * |a - exact|_2 <= sum_i weights[i] (e_{k+i} + (L + 1) eps), likewise b; with d = a - b and E = the two of them + eps |d|_2,
 * |novelty - exact| <= 2 |d|_2 E + E^2 + 8 eps novelty (tests/sections_ref.py computes exactly this from the inputs).  The bound
 * grows with mean|B[k]| / |x|_2: a nearly constant row has no direction to speak of.
 * A track whose range is negative or runs outside [0, total] (r0 < 0, r1 < r0, r1 > total) is skipped: nothing of it is read or
 * written and its neighbours are unaffected.  A workgroup of sixteen waves takes 64 beats of one track: the tile's rows and L rows
 * either side are normalised into LDS once, a wave taking two rows at a time, ((64 + 2 L) * 512 bytes of dynamic LDS: 96 KB at L =
 * 64, 48 KB at L = 16); then a wave per beat walks the 2 L rows of LDS.  A track of any length is walked tile by tile (grid (N, min(ceil(total / 64),
 * 1024)), a block striding over the rest).  No atomics, no workspace, no scratch.  N == 0 or total == 0 is a no-op.  Refused before
 * any launch: negative sizes, L outside [1, 64], N or total >= 2^31, a null pointer with total > 0. */
int made_section_novelty(const float* B, const int64_t* beat_start, int64_t N, int64_t total, const float* weights, int32_t L,
                         float* novelty, void* stream);

/* made_section_pick: the boundaries of N tracks from their novelty.  novelty [total] f32, beat_start as above, time [N, cap] f32 the
 * beat times (made_beat_track's), metre / phase [N] device int32 or both NULL (made_bar_pick's), 1 <= L <= 64 (the novelty's), 1 <=
 * w <= 256, thresh_factor and floor finite f32.  Outputs bound_time / bound_strength [N, cap_s] f32, bound_beat [N, cap_s] int32,
 * bound_count [N] int32, mean [N] f32.  Every step is one rounded f32 operation.  Per track:
 *   1. The candidates are the beats k with L <= k <= n - L; when metre != NULL and metre[t] > 0 only those with (k - phase[t]) mod
 *      metre[t] == 0 (the mathematical, non-negative remainder): a section starts on a bar line when the track has one.
 *   2. mean[t] = (novelty summed over the candidates: one chain, ascending, from +0) / (float)(their number); NaN without candidates.
 *   3. thresh = mean[t] * thresh_factor (the host passes 1 + delta).  Candidate k with x = novelty[k] is a boundary iff x > 0, x >
 *      novelty[j] for every candidate j in [k - w, k), x >= novelty[j] for every candidate j in (k, k + w], x >= floor and x >= thresh.
 *      Of equal neighbours the earlier wins; a NaN anywhere in the window, or a NaN mean, makes no boundary.  Two boundaries are
 *      therefore at least w + 1 beats apart, no greedy
 *      pass is needed and the rule is decided per beat.
 *   4. The boundaries are written ascending in k: bound_time[t * cap_s + i] = time[t * cap + k] (the beat's own f32 time), bound_beat =
 *      k, bound_strength = x / mean[t].  bound_count[t] = their number; entries from bound_count on are not written.  A track with
 *      more than cap_s boundaries gets bound_count = -1 (its first cap_s entries hold its first cap_s boundaries).  cap_s >=
 *      ceil(cap / (w + 1)) cannot overflow.
 * A track whose list does not fit its arrays (n < 0, n > cap, rows outside [0, total]) gets bound_count = -1 and mean = NaN, and
 * nothing of it is read.  One workgroup of four waves per track: the novelty is staged through LDS 1024 beats at a time, one thread
 * walks the chain of step 2, then every thread decides beats of step 3 and each quarter of a pass is compacted in beat order -- a
 * ballot and a prefix popcount inside the wave, the waves' counts through LDS, a running offset -- as made_onset_peaks does.  No
 * atomics, no workspace, no scratch.  N == 0 is a no-op.  Refused: negative sizes, L outside [1, 64], w outside [1, 256], a
 * thresh_factor or floor that is not finite, metre without phase, N or total >= 2^31, null pointers (novelty may be NULL when total
 * == 0, time when cap == 0, the three lists when cap_s == 0). */
int made_section_pick(const float* novelty, const int64_t* beat_start, const float* time, int64_t cap, int64_t N, int64_t total,
                      const int32_t* metre, const int32_t* phase, int32_t L, int32_t w, float thresh_factor, float floor, float* bound_time,
                      int32_t* bound_beat, float* bound_strength, int64_t cap_s, int32_t* bound_count, float* mean, void* stream);

/* ---- Cuts (mgsv_amd/cuts.py; csrc/cuts.hip) -------------------------------------------------------------------------------------
 * Where a video's shots change, from its decoded frames: the list made_sync_moments takes as cut_start / cut_time.  A video is F
 * frames of one size H x W, RGB uint8 interleaved [H, W, 3]; P = H * W, 1 <= P <= 2^24; videos of mixed sizes may share a call.
 * Everything below is integer arithmetic, every division an integer floor division: no order of additions can change a bit.
 * The reference has no counterpart.
 *
 * Signature (made_frame_hist).  For the pixel at row r, column c of frame f:
 *   1. luma Y = (77 R + 150 G + 29 B + 128) >> 8                       (0 .. 255);
 *   2. bin b = Y >> 2                                                  (64 bins);
 *   3. cell = 4 * (4 r / H) + (4 c / W)                                (a 4 x 4 grid; cells are empty when H or W is below 4).
 * hist[f, cell, b] (uint32 [n_frames, 16, 64]) counts the pixels of frame f with that cell and bin; a frame's counts sum to P.
 *
 * Distance (made_hist_distance).  D[0] = 0; D[f] = sum over cell, b of |hist[f] - hist[f - 1]| (uint32), so 0 <= D[f] <= 2 P; a
 * frame whose first_of_video flag is set (the first frame of every video, wherever it sits in the batch) has D = 0.
 *
 * Pick (made_cut_peaks).  Frame f of video v (F = n_frames[v] frames, D = its row) is a cut iff, in int64 arithmetic,
 *   1. D[f] >= thr[v] and D[f] > 0 (thr a per-video device uint32: the host's ceil(threshold * 2 P));
 *   2. D[f] > D[g] for g in [f - w_max, f) and D[f] >= D[g] for g in (f, f + w_max], the windows clipped to [0, F): of equal
 *      neighbours the earlier wins;
 *   3. 256 * D[f] * n >= ratio_q8 * S, S the sum of D over [f - w_avg, f + w_avg] clipped to [1, F) without f itself and n the
 *      number of frames in it (D[0] is 0 by definition, not a measurement: it is left out); with n == 0 the test passes.  This
 *      rejects sustained motion and shake, where every distance is large -- and a real cut inside such a stretch.
 * ------------------------------------------------------------------------------------------------------------------------------- */

/* One frame of made_frame_hist's packed input. */
typedef struct MadeCutFrameDesc {
    int64_t offset;        /* byte offset of the frame's first pixel in `frames` (RGB, 3 bytes per pixel, rows of 3 W bytes, no gaps) */
    int32_t H, W;          /* rows and columns */
} MadeCutFrameDesc;

/* made_frame_hist: the signatures of n_frames frames.  frames: device bytes, frames_len of them; desc [n_frames] device array;
 * hist [n_frames, 16, 64] uint32, every word of which is written (zeroed by an asynchronous memset on the stream, then counted
 * into) and nothing beyond.  A frame is one contiguous byte range; a workgroup takes chunks of 16 384 consecutive pixels, a lane
 * 16 pixels (48 bytes) at a time: three 16-byte loads when the frame's first byte is 16-byte aligned, twelve dword loads when it
 * is 4-byte aligned, byte loads otherwise and for the frame's last partial step -- all fill the same twelve words, so the counts
 * do not depend on the path; nothing outside [offset, offset + 3 P) is read.  (r, c) comes from one division per lane and step,
 * then an increment with wrap (with W >= 64 the 16 pixels change their cell once at most, which is looked up once).  A lane merges
 * runs of equal (cell, bin) among its 16 pixels into one add of the run's length, to the wave's own 1024-word LDS histogram (folding
 * the lanes of a wave that share a target bought nothing on top of that and was taken out).  The workgroups of a frame (ceil(mean P /
 * 16 384) each, from frames_len / n_frames: the host cannot see the descriptors) add their non-zero counts into hist with integer
 * global atomics.  A descriptor with H or W < 1, P > 2^24, offset < 0 or offset + 3 P > frames_len leaves a zero signature and
 * reads nothing.  n_frames == 0 is a no-op.  Refused: negative sizes, n_frames >= 2^21, frames_len < 3, null pointers. */
int made_frame_hist(const uint8_t* frames, int64_t frames_len, const MadeCutFrameDesc* desc, int64_t n_frames, uint32_t* hist,
                    void* stream);

/* made_hist_distance: D [n_frames] uint32 of hist [n_frames, 16, 64] uint32 (16-byte aligned) by the rule above; first_of_video
 * [n_frames] device uint8, non-zero forces D = 0 (frame 0 needs no flag).  One wave per frame: four 16-byte loads of either
 * signature per lane, an integer DPP sum.  No LDS, no atomics.  n_frames == 0 is a no-op.  Refused: a negative n_frames or one
 * >= 2^31, null pointers, a hist that is not 16-byte aligned. */
int made_hist_distance(const uint32_t* hist, const uint8_t* first_of_video, int64_t n_frames, uint32_t* D, void* stream);

/* made_cut_peaks: the cuts of N videos from their distances D [N, D_ld] uint32 by the rule above; n_frames [N] device int32, thr
 * [N] device uint32.  count[v] int32 = the number of cuts; frame[v * cap + i] int32, i < count[v] = the cut frames ascending;
 * strength[v * cap + i] uint32 = D[frame].  Entries from count[v] on are not written.  Rule 2 keeps two cuts w_max + 1 frames
 * apart, so cap >= ceil(D_ld / (w_max + 1)) never overflows (a smaller cap is refused).  One workgroup per video walks tiles of
 * 1024 frames with a 128-frame halo in LDS; the compaction is ordered (ballot, prefix popcount, a running offset): no atomics, no
 * workspace, and a video's list does not depend on the other videos.  A video with n_frames[v] > D_ld (or < 0) gets count -1 and
 * no entries.  w_max in [1, 64], w_avg in [1, 128], ratio_q8 in [0, 65535]; N == 0 is a no-op.  Refused: those ranges, negative
 * sizes, N or D_ld >= 2^31, null pointers (D may be NULL when D_ld == 0, frame and strength when cap == 0). */
int made_cut_peaks(const uint32_t* D, int64_t D_ld, const int32_t* n_frames, int64_t N, const uint32_t* thr, int32_t w_max,
                   int32_t w_avg, int32_t ratio_q8, int64_t cap, int32_t* frame, uint32_t* strength, int32_t* count, void* stream);

/* ==========================================================================================
 * Batches from a device-resident feature store (mgsv_amd/feature_store.py DeviceFeatureStore): a split's features stay on the
 * device in their storage format and every batch of the training / evaluation loop is assembled by one launch.  The reference
 * loads four files per sample in worker processes (dataloaders/dataloader_MGSV_EC_feature.py:57-67).
 * ========================================================================================== */

#define MADE_GATHER_MAX_ARRAYS 8
enum MadeGatherKind { MADE_GATHER_F32 = 0, MADE_GATHER_BF16 = 1, MADE_GATHER_U8 = 2 };

/* One array of made_gather_batch.  src [rows, row_elems] contiguous rows of `kind`; row [n_samples] device int32 (sample s reads
 * row row[s]) or NULL (sample s reads row s); dst [B, row_elems] contiguous f32. */
typedef struct MadeGatherArray {
    const void*    src;
    const int32_t* row;
    float*         dst;
    int64_t        rows;
    int64_t        row_elems;
    int32_t        kind;       /* MadeGatherKind */
    int32_t        _pad;
} MadeGatherArray;

typedef struct MadeGatherBatchArgs {
    MadeGatherArray a[MADE_GATHER_MAX_ARRAYS];
    const int32_t*  index;     /* [B] device int32: the batch's sample numbers */
    int64_t         n_samples;
    int64_t         B;
    int32_t         n_arrays;  /* 1 .. MADE_GATHER_MAX_ARRAYS */
    int32_t         _pad;
} MadeGatherBatchArgs;

/* made_gather_batch: for every b < B and array a, with s = index[b] and r = row_a ? row_a[s] : s:
 *     dst_a[b, :] = widen(src_a[r, :])   if 0 <= s < n_samples and 0 <= r < rows_a,   a zero row (nothing is read) otherwise
 * -- made_gather_rows' rule.  widen is exact: f32 the same 32 bits (copied as integers: NaN payloads and -0 survive), bf16 the
 * pattern << 16, u8 (float)v.  One launch; the descriptors travel in the kernel's arguments (no upload, no host sync).  Grid:
 * y = the array, x = (sample, piece of the row), so one long row is spread over the chip.  Per array the launcher takes the
 * 16-byte path (one 16-byte load per lane; one, two or four 16-byte stores for f32, bf16, u8) when the row's source bytes are a
 * multiple of 16 and src and dst are 16-byte aligned, and the element path (one element per lane) otherwise; both give the same
 * bits.  No LDS, no atomics, no workspace.  B == 0 is a no-op; an array with row_elems == 0 is skipped.  Refused: null args /
 * index / src (with rows > 0) / dst, n_arrays outside [1, 8], negative sizes, rows, n_samples or B past 2^31, B * row_elems of
 * one array past 2^31, pointers not aligned to their element, a dst that overlaps its src. */
int made_gather_batch(const MadeGatherBatchArgs* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MADE_HIP_H */
