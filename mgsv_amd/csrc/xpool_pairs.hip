// made_xpool_sims_pairs: the X-Pool score of LISTED (video, track) pairs -- made_xpool_sims' arithmetic (scores by MFMA, masked softmax in f32,
// probabilities rounded to bf16 before the two P.V products, y = k1 z + k2 Bv + Av, LayerNorm3 and the cosine through the six sums) for the pairs
// of a CSR: per distinct track the ascending list of the videos that shortlisted it (grounding.py, `ground(..., shortlist=R)`).  gfx950, bf16,
// D = 256, tracks of at most 96 segments.
//
// A workgroup (four waves) takes ONE track and tiles of 32 of its listed videos (tile blockIdx.y, then every gridDim.y-th).  The track's value
// rows u | u'' go through LDS once per workgroup, TRANSPOSED on the way in (row d of the LDS copy holds u[., d] over the segments), so that the
// A operand of the second product -- 8 consecutive segments of one value column -- is one 16-byte LDS read and nothing needs the transposing
// LDS instructions; rows of masked segments are stored as zeros.  The track's K rows are the A operand of the score product as they lie in
// memory (8 consecutive columns of one segment) and each of them is used by exactly one wave, so they are read straight into registers.  Q rows
// and the per-video terms (vn, from which g3 vn, sum g3 vn and sum b3 vn are formed in the tail) are gathered by the listed video index: there is
// no workspace and no preparation launch, and nothing of a pair depends on which other pairs share its tile or its launch -- a video's values
// live in one MFMA column / one lane pair, and every sum runs in an order fixed by the lane, not by the slot.
//   wave w:  scores of segments [32 w, 32 w + 32) for the tile's 32 videos; rows [64 w, 64 w + 64) of o and of z in the second product and the tail.
#include "common.h"

namespace {

constexpr int XD = 256;                 // model width
constexpr int XS = 96;                  // segments per track at most
constexpr int XQ = 32;                  // videos per tile
constexpr int XT = 256;                 // threads
constexpr int UT_LD = XS + 8;           // bf16 elements per row of the transposed value tile / of the probability tile (208 B: 16-byte aligned rows)
constexpr int OFF_UT = 0;                                   // [2 D][UT_LD] bf16: u^T | u''^T
constexpr int OFF_P = OFF_UT + 2 * XD * UT_LD * 2;          // [32 videos][UT_LD] bf16 probabilities
constexpr int OFF_VEC = OFF_P + XQ * UT_LD * 2;             // [6][D] f32: Av, Bv, g3^2, g3 b3, g3, b3
constexpr int OFF_MAX = OFF_VEC + 6 * XD * 4;               // [4 waves][32] f32
constexpr int OFF_SUM = OFF_MAX + 4 * XQ * 4;               // [4][32] f32
constexpr int OFF_ST = OFF_SUM + 4 * XQ * 4;                // [4][32][2] f32: a wave's part of LayerNorm2's sums
constexpr int OFF_PART = OFF_ST + 4 * XQ * 8;               // [4][32][8] f32: a wave's part of the tail's sums
constexpr int OFF_BIAS = OFF_PART + 4 * XQ * 32;            // [96] f32: 0 for a valid segment, -inf otherwise
constexpr int OFF_C = OFF_BIAS + XS * 4;                    // sum g3^2, sum g3 b3, sum b3^2
constexpr int LDS_BYTES = OFF_C + 16;
static_assert(LDS_BYTES <= 160 * 1024, "made_xpool_sims_pairs: the LDS map does not fit a CU");
static_assert((UT_LD * 2) % 16 == 0 && OFF_P % 16 == 0 && OFF_VEC % 16 == 0, "16-byte aligned rows");

__device__ __forceinline__ float other_half(float x) { return __shfl_xor(x, 32); }

__global__ __launch_bounds__(XT) void xpool_pairs_kernel(const MadeXpoolPairsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int64_t u = blockIdx.x;
    int64_t p0 = a.start[u], p1 = a.start[u + 1];
    p0 = p0 < 0 ? 0 : (p0 > a.P ? a.P : p0);
    p1 = p1 < p0 ? p0 : (p1 > a.P ? a.P : p1);
    const int count = (int)(p1 - p0);
    if ((int64_t)blockIdx.y * XQ >= count) return;               // (uniform: an empty range, or fewer tiles than the longest list)
    const int S = (int)a.S;
    const int S16 = (S + 15) & ~15;
    const int ntiles = (S + 31) >> 5;

    bf16_t* ut = (bf16_t*)(lds + OFF_UT);
    bf16_t* pl = (bf16_t*)(lds + OFF_P);
    float* vec = (float*)(lds + OFF_VEC);
    float* lmax = (float*)(lds + OFF_MAX);
    float* lsum = (float*)(lds + OFF_SUM);
    float* lst = (float*)(lds + OFF_ST);
    float* part = (float*)(lds + OFF_PART);
    float* bias = (float*)(lds + OFF_BIAS);
    float* cst = (float*)(lds + OFF_C);

    // ---- the track: segment validity, the model's vectors, the transposed value rows
    if (tid < XS) {
        const bool valid = tid < S && (a.key_mask == nullptr || a.key_mask[u * a.S + tid] != 0.f);
        bias[tid] = valid ? 0.f : -INFINITY;
    }
    {
        const float g3 = a.ln3_g[tid], b3 = a.ln3_b[tid];         // (256 threads = D)
        vec[tid] = a.av[tid]; vec[XD + tid] = a.bv[tid]; vec[2 * XD + tid] = g3 * g3; vec[3 * XD + tid] = g3 * b3;
        vec[4 * XD + tid] = g3; vec[5 * XD + tid] = b3;
    }
    if (wave == 0) {
        float c0 = 0.f, e0 = 0.f, f0 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = a.ln3_g[lane * 4 + j], b = a.ln3_b[lane * 4 + j];
            c0 += g * g; e0 += g * b; f0 += b * b;
        }
#pragma unroll
        for (int o2 = 32; o2 > 0; o2 >>= 1) { c0 += __shfl_xor(c0, o2); e0 += __shfl_xor(e0, o2); f0 += __shfl_xor(f0, o2); }
        if (lane == 0) { cst[0] = c0; cst[1] = e0; cst[2] = f0; }
    }
    __syncthreads();
    {
        const bf16_t* ub = (const bf16_t*)a.UU + u * a.u_bs;
        const int items = (S16 >> 1) * (2 * XD / 8);              // (pair of segments, 8 value columns)
        for (int it = tid; it < items; it += XT) {
            const int sp = it >> 6, c = it & 63;
            const int s0 = 2 * sp;
            bf16x8 x0, x1;
#pragma unroll
            for (int j = 0; j < 8; ++j) { x0[j] = (bf16_t)0.f; x1[j] = (bf16_t)0.f; }
            if (s0 < S && bias[s0] == 0.f) x0 = *(const bf16x8*)(ub + (int64_t)s0 * a.ldu + c * 8);
            if (s0 + 1 < S && bias[s0 + 1] == 0.f) x1 = *(const bf16x8*)(ub + (int64_t)(s0 + 1) * a.ldu + c * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                bf16_t* d = ut + (c * 8 + j) * UT_LD + s0;
                d[0] = x0[j]; d[1] = x1[j];
            }
        }
    }
    __syncthreads();

    const float c = a.scale * 1.4426950408889634f;
    const bf16_t* kb = (const bf16_t*)a.K + u * a.k_bs;
    const int seg = 32 * wave + r;                                // the K row this lane feeds to the score product
    const bool kvalid = wave < ntiles && seg < S && bias[seg] == 0.f;

    for (int t = blockIdx.y; (int64_t)t * XQ < count; t += gridDim.y) {
        const int slot = t * XQ + r;
        const bool has = slot < count;
        const int64_t v = has ? (int64_t)a.video[p0 + slot] : -1;
        const bool ok = has && v >= 0 && v < a.Nv;                // (anything else reads nothing of Q / vn)

        // ================================================================================ scores of K tile `wave`, softmax over the track
        f32x16 sacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
        float mx = -INFINITY;
        if (wave < ntiles) {
            const bf16_t* kp = kb + (int64_t)(kvalid ? seg : 0) * a.ldk + hh * 8;
            const bf16_t* qp = (const bf16_t*)a.Q + (ok ? v : 0) * a.ldq + hh * 8;
#pragma unroll
            for (int ks = 0; ks < XD / 16; ++ks) {
                bf16x8 kf, qf;
#pragma unroll
                for (int j = 0; j < 8; ++j) { kf[j] = (bf16_t)0.f; qf[j] = (bf16_t)0.f; }
                if (kvalid) kf = *(const bf16x8*)(kp + ks * 16);
                if (ok) qf = *(const bf16x8*)(qp + ks * 16);
                sacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf, sacc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                sacc[e] = sacc[e] * c + bias[32 * wave + acc_row(e, hh)];
                mx = fmaxf(mx, sacc[e]);
            }
        }
        mx = fmaxf(mx, other_half(mx));
        if (hh == 0) lmax[wave * XQ + r] = mx;
        __syncthreads();
        float M = lmax[r];
#pragma unroll
        for (int q = 1; q < 4; ++q) M = fmaxf(M, lmax[q * XQ + r]);
        float psum = 0.f;
        if (wave < ntiles) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 pf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float pr = __builtin_amdgcn_exp2f(sacc[4 * g + j] - M);      // (no valid segment: -inf - -inf = NaN, like the dense kernel)
                    psum += pr;
                    pf[j] = (bf16_t)pr;
                }
                *(bf16x4*)(pl + r * UT_LD + 32 * wave + 8 * g + 4 * hh) = pf;
            }
        }
        psum += other_half(psum);
        if (hh == 0) lsum[wave * XQ + r] = psum;
        __syncthreads();

        // ================================================================================ [O | Z]^T = [U | U'']^T P^T, 16 segments per step
        float l = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) l += lsum[q * XQ + r];
        const float inv_l = 1.f / l;
        f32x16 oacc[4];                                           // [0], [1]: rows 64 w .., 64 w + 32 .. of o; [2], [3]: the same rows of z
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[dt][e] = 0.f;
        for (int k0 = 0; k0 < S16; k0 += 16) {
            const bf16x8 pb = *(const bf16x8*)(pl + r * UT_LD + k0 + hh * 8);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const int d0 = (dt >> 1) * XD + 64 * wave + 32 * (dt & 1);
                const bf16x8 uf = *(const bf16x8*)(ut + (d0 + r) * UT_LD + k0 + hh * 8);
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(uf, pb, oacc[dt], 0, 0, 0);
            }
        }
        // LayerNorm2's statistics of o / l: this wave's 64 rows
        {
            float su = 0.f, sq = 0.f;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float x = oacc[dt][e] * inv_l;
                    su += x; sq += x * x;
                }
            su += other_half(su); sq += other_half(sq);
            if (hh == 0) { lst[(wave * XQ + r) * 2] = su; lst[(wave * XQ + r) * 2 + 1] = sq; }
        }
        __syncthreads();
        float su = 0.f, sq = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) { su += lst[(q * XQ + r) * 2]; sq += lst[(q * XQ + r) * 2 + 1]; }
        const float mean2 = su * (1.f / XD);
        const float var2 = fmaxf(sq * (1.f / XD) - mean2 * mean2, 0.f);
        const float k1 = __builtin_amdgcn_rsqf(var2 + a.eps), k2 = -mean2 * k1;

        // ================================================================================ tail: y = k1 z + k2 Bv + Av, the sums of LayerNorm3 + cosine
        {
            float s1 = 0.f, s2 = 0.f, p1 = 0.f, c2 = 0.f, c1 = 0.f, e1 = 0.f, gs = 0.f, bs = 0.f;
            const float* vp = a.vn + (ok ? v : 0) * a.ldvn;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = 64 * wave + 32 * j + 8 * g + 4 * hh;
                    f32x4 vn4 = {0.f, 0.f, 0.f, 0.f};
                    if (ok) vn4 = *(const f32x4*)(vp + d);
                    const f32x4 av4 = *(const f32x4*)(vec + d), bv4 = *(const f32x4*)(vec + XD + d), g24 = *(const f32x4*)(vec + 2 * XD + d);
                    const f32x4 gb4 = *(const f32x4*)(vec + 3 * XD + d), g34 = *(const f32x4*)(vec + 4 * XD + d), b34 = *(const f32x4*)(vec + 5 * XD + d);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float z = oacc[2 + j][4 * g + i] * inv_l;
                        const float y = k1 * z + (k2 * bv4[i] + av4[i]);
                        const float gv = g34[i] * vn4[i];
                        const float yy = y * y;
                        s1 += y; s2 += yy; p1 += y * gv; c2 += yy * g24[i]; c1 += y * g24[i]; e1 += y * gb4[i];
                        gs += gv; bs += b34[i] * vn4[i];
                    }
                }
            s1 += other_half(s1); s2 += other_half(s2); p1 += other_half(p1); c2 += other_half(c2);
            c1 += other_half(c1); e1 += other_half(e1); gs += other_half(gs); bs += other_half(bs);
            if (hh == 0) {
                float* pw = part + (wave * XQ + r) * 8;
                *(f32x4*)pw = (f32x4){s1, s2, p1, c2};
                *(f32x4*)(pw + 4) = (f32x4){c1, e1, gs, bs};
            }
        }
        __syncthreads();
        if (wave == 0 && hh == 0 && has) {
            f32x4 A0 = *(const f32x4*)(part + r * 8), A1 = *(const f32x4*)(part + r * 8 + 4);
#pragma unroll
            for (int q = 1; q < 4; ++q) { A0 += *(const f32x4*)(part + (q * XQ + r) * 8); A1 += *(const f32x4*)(part + (q * XQ + r) * 8 + 4); }
            const float s1 = A0[0], s2 = A0[1], p1 = A0[2], c2 = A0[3], c1 = A1[0], e1 = A1[1], pg = A1[2], pb = A1[3];
            const float mu = s1 * (1.f / XD);
            const float var = fmaxf(s2 * (1.f / XD) - mu * mu, 0.f);
            const float rs = __builtin_amdgcn_rsqf(var + a.eps);
            const float dot = rs * (p1 - mu * pg) + pb;
            const float zz = rs * rs * (c2 - 2.f * mu * c1 + mu * mu * cst[0]) + 2.f * rs * (e1 - mu * cst[1]) + cst[2];
            a.score[p0 + slot] = ok ? dot * __builtin_amdgcn_rsqf(zz) : __uint_as_float(0x7FC00000u);
        }
        // (the next tile's first LDS write -- lmax -- is behind this tile's reads of it by three barriers; `part` is rewritten only after the
        //  next tile's three barriers, which wave 0 joins after the reads above)
    }
}

}  // namespace

extern "C" int made_xpool_sims_pairs(const MadeXpoolPairsArgs* args, void* stream) {
    MADE_REQUIRE(args != nullptr, "made_xpool_sims_pairs: null args");
    const MadeXpoolPairsArgs& a = *args;
    MADE_REQUIRE(a.U >= 0 && a.P >= 0 && a.Nv >= 0 && a.S > 0 && a.U < (1LL << 31) && a.P < (1LL << 31), "made_xpool_sims_pairs: bad dims");
    if (a.U == 0) return MADE_OK;
    MADE_REQUIRE(a.start != nullptr, "made_xpool_sims_pairs: null pointer (start)");
    if (a.P == 0) return MADE_OK;
    MADE_REQUIRE(a.K && a.UU && a.av && a.bv && a.ln3_g && a.ln3_b && a.video && a.score && (a.Nv == 0 || (a.Q && a.vn)),
                 "made_xpool_sims_pairs: null pointer");
    MADE_UNSUPPORTED(a.D == XD, "made_xpool_sims_pairs: D=%lld (built for %d)", (long long)a.D, XD);
    MADE_UNSUPPORTED(a.S <= XS, "made_xpool_sims_pairs: S=%lld segments per track (at most %d)", (long long)a.S, XS);
    MADE_UNSUPPORTED(a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldu % 8 == 0 && a.k_bs % 8 == 0 && a.u_bs % 8 == 0 && a.ldvn % 4 == 0 &&
                     ((uintptr_t)a.Q % 16) == 0 && ((uintptr_t)a.K % 16) == 0 && ((uintptr_t)a.UU % 16) == 0 && ((uintptr_t)a.vn % 16) == 0,
                     "made_xpool_sims_pairs: pointers / strides must keep 16-byte alignment");
    MADE_UNSUPPORTED(a.ldq >= XD && a.ldk >= XD && a.ldu >= 2 * XD && a.ldvn >= XD && a.k_bs >= 0 && a.u_bs >= 0,
                     "made_xpool_sims_pairs: rows shorter than the model width (value rows hold u | u'': ldu >= 2 D)");
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)xpool_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
        if (e != hipSuccess) { made_set_error("made_xpool_sims_pairs: cannot reserve %d bytes of LDS: %s", LDS_BYTES, hipGetErrorString(e)); return MADE_ERR_HIP; }
        attr_done = true;
    }
    int64_t longest = a.max_count > 0 ? a.max_count : a.P;       // (tiles beyond the grid are walked by the tile loop)
    if (longest > a.P) longest = a.P;
    int64_t gy = (longest + XQ - 1) / XQ;
    if (gy < 1) gy = 1;
    if (gy > 1024) gy = 1024;
    hipLaunchKernelGGL(xpool_pairs_kernel, dim3((unsigned)a.U, (unsigned)gy), dim3(XT), LDS_BYTES, (hipStream_t)stream, a);
    return made_check_launch("made_xpool_sims_pairs");
}
