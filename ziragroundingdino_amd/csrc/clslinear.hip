// clslinear.hip -- the trained class head of the linear-probing baseline, forward and backward: cls_linear, the product with the
// text and the fold of token logits into category logits as one pass (C ABI and the defining formulas: include/zira_clslinear.h;
// reference models/GroundingDINO/utils.py:272-320).
//
// One wave -- a block of its own -- owns 32 rows of ONE image of one prediction set (the rows of an image's Q queries are dealt in
// blocks of 32, the last one partly filled), so every product of the wave is with that image's text.  Every product is
// v_mfma_f32_32x32x2_f32 with fp32 accumulation, and every matrix is kept TRANSPOSED in the accumulators -- the row on the lane,
// the feature (or token) index in the registers: an accumulator tile is then the B operand of the next product as it stands
// (the instruction's reduction index is free as long as both operands agree on it: csrc/mfma_f32_tile.h), with no trip through LDS.
//
// forward   zT = W xT + bias (eight 32 x 32 tiles: the 256 features of the wave's rows, 128 registers);  per panel of 32 tokens
//           lT = text zT, the text rows read straight from global memory (L2-resident: 256 KB per image at most) in the feature
//           order the accumulator registers hold -- the text is STREAMED in panels of 32 tokens through registers, nothing of it
//           is staged;  the panel's logits go to the wave's [token][row] LDS tile (32 KB at 256 tokens);  then a lane per row and
//           half wave per category parity scans each category's token range in token order (cat_max.h).  Neither z nor the token
//           logits reach memory.
// backward  the rows' category gradients are scattered into a [token][row] LDS tile (one token per category: the arg table);
//           gzT = textT glT on the matrix cores, skipping token pairs no row of the wave uses;  gz rows and their column sums
//           (a double per block and column; the last block to arrive -- integer ticket -- adds them in index order) leave the
//           wave;  gxT = WT gzT from the accumulators when asked for.  g_W = gz^T x is zira_xty_f32's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "cat_max.h"
#include "launch.h"
#include "mfma_f32_tile.h"
#include "zira_clslinear.h"
#include "zira_msda.h"

namespace {

constexpr int kD = 256, kTiles = kD / 32, kRows = 32, kThreads = 64, kMaxT = 256, kMaxC = 256;
constexpr long long kMaxR = 1ll << 22;
using zira::align4, zira::misaligned;

// the wave's place: block -> (prediction set and image, block of 32 queries)
struct Place {
    int b, nrows;
    long long row0;
};
__device__ __forceinline__ Place place_of(unsigned block, int B, int Q)
{
    const int bps = (Q + kRows - 1) / kRows;
    const long long seg = block / bps;
    const int q0 = (int)(block % bps) * kRows;
    Place p;
    p.b = (int)(seg % B);
    p.nrows = Q - q0 < kRows ? Q - q0 : kRows;
    p.row0 = seg * Q + q0;
    return p;
}

__global__ __launch_bounds__(kThreads) void cls_linear_fwd(const float *__restrict__ x, const float *__restrict__ W,
                                                           const float *__restrict__ bias, const float *__restrict__ text,
                                                           const uint8_t *__restrict__ tok_mask, const uint8_t *__restrict__ cat_mask,
                                                           const int32_t *__restrict__ cat_range, const int32_t *__restrict__ n_cat,
                                                           const int32_t *__restrict__ n_tok, int B, int Q, int T, int T_out, int Cmax,
                                                           int Tmax, float for_fill, float *__restrict__ out,
                                                           int32_t *__restrict__ arg)
{
    __shared__ float lt[kMaxT * kRows];      // the token logits of the wave's rows, [token][row]

    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const Place p = place_of(blockIdx.x, B, Q);
    const int b = p.b;
    const long long rowc = p.row0 + (r < p.nrows ? r : p.nrows - 1);      // (rows beyond the block: clamped for the loads, never stored)
    int nc = n_cat[b], nt = n_tok[b];
    nc = nc < 0 ? 0 : (nc > Cmax ? Cmax : nc);
    nt = nt > T ? T : nt;
    nt = nt > Tmax ? Tmax : nt;
    nt = nt < 0 ? 0 : nt;

    if (nc > 0 && nt > 0) {
        // ---- zT = W xT + bias: lane (r, hh), register reg of tile j holds z[row r][32 j + rowmap(reg, hh)] ---------------------------
        f32x16 acc[kTiles];
#pragma unroll
        for (int j = 0; j < kTiles; ++j) acc[j] = zero16();
#pragma unroll
        for (int c = 0; c < kD / 64; ++c) {
            const int k0 = 64 * c + 32 * hh;
            float xa[32];
            load_floats(x + (size_t)rowc * kD + k0, xa);
#pragma unroll
            for (int j = 0; j < kTiles; ++j) {
                float wb[32];
                load_floats(W + (size_t)(32 * j + r) * kD + k0, wb);
                mfma_chain<32>(wb, xa, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < kTiles; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 bv = *reinterpret_cast<const float4 *>(bias + 32 * j + 8 * g + 4 * hh);
                acc[j][4 * g] += bv.x; acc[j][4 * g + 1] += bv.y; acc[j][4 * g + 2] += bv.z; acc[j][4 * g + 3] += bv.w;
            }

        // ---- per panel of 32 tokens: lT = text zT; the text in the accumulators' feature order --------------------------------------
        const float *tb = text + (size_t)b * T * kD;
#pragma unroll 1
        for (int t0 = 0; t0 < nt; t0 += 32) {
            const int tl = t0 + r < nt ? t0 + r : nt - 1;
            const float *tr = tb + (size_t)tl * kD + 4 * hh;
            f32x16 l = zero16();
#pragma unroll
            for (int j = 0; j < kTiles; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 tv = *reinterpret_cast<const float4 *>(tr + 32 * j + 8 * g);
                    l = __builtin_amdgcn_mfma_f32_32x32x2f32(tv.x, acc[j][4 * g], l, 0, 0, 0);
                    l = __builtin_amdgcn_mfma_f32_32x32x2f32(tv.y, acc[j][4 * g + 1], l, 0, 0, 0);
                    l = __builtin_amdgcn_mfma_f32_32x32x2f32(tv.z, acc[j][4 * g + 2], l, 0, 0, 0);
                    l = __builtin_amdgcn_mfma_f32_32x32x2f32(tv.w, acc[j][4 * g + 3], l, 0, 0, 0);
                }
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int t = t0 + rowmap(reg, hh);
                if (t < kMaxT) lt[t * kRows + r] = l[reg];
            }
        }
    }
    __syncthreads();

    // ---- a lane per row, a half wave per category parity: the category's tokens in token order ---------------------------------------
    if (r < p.nrows) {
        const long long row = p.row0 + r;
        const uint8_t *tm = tok_mask + (size_t)b * T;
        for (int c = hh; c < nc; c += 2) {
            const int32_t *rg = cat_range + ((size_t)b * Cmax + c) * 2;
            const uint8_t *cm = cat_mask + ((size_t)b * Cmax + c) * Tmax;
            int lo = rg[0], hi = rg[1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > nt ? nt : hi;
            float best = -INFINITY;
            int at = -1;
            for (int t = lo; t < hi; ++t) zira_cat_max_step(cm[t] != 0 && tm[t] != 0, lt[t * kRows + r], t, best, at);
            out[row * T_out + c] = zira_cat_max_value(best, at, for_fill);
            arg[row * Cmax + c] = at;
        }
    }
    // ---- everything beyond the image's categories --------------------------------------------------------------------------------------
    for (int rr = 0; rr < p.nrows; ++rr) {
        const long long row = p.row0 + rr;
        for (int c = nc + lane; c < T_out; c += kThreads) out[row * T_out + c] = for_fill;
        for (int c = nc + lane; c < Cmax; c += kThreads) arg[row * Cmax + c] = -1;
    }
}

__global__ __launch_bounds__(kThreads) void cls_linear_bwd(const float *__restrict__ gout, const int32_t *__restrict__ arg,
                                                           const int32_t *__restrict__ n_cat, const int32_t *__restrict__ n_tok,
                                                           const float *__restrict__ W, const float *__restrict__ text, int B, int Q,
                                                           int T, int T_out, int Cmax, float *__restrict__ gz, float *__restrict__ gx,
                                                           double *part, unsigned *counter, float *__restrict__ g_b)
{
    __shared__ float gl[kMaxT * kRows];      // the rows' token-logit gradients, [token][row]: one token per category
    __shared__ int is_last;

    const int lane = threadIdx.x, r = lane & 31, hh = lane >> 5;
    const Place p = place_of(blockIdx.x, B, Q);
    const int b = p.b;
    const bool valid = r < p.nrows;
    const long long row = p.row0 + (valid ? r : p.nrows - 1);
    int nc = n_cat[b], nt = n_tok[b];
    nc = nc < 0 ? 0 : (nc > Cmax ? Cmax : nc);
    nt = nt > T ? T : nt;
    nt = nt < 0 ? 0 : nt;
    const int nt2 = (nt + 1) & ~1;           // (<= 256: T <= 256)

    for (int i = lane; i < nt2 * kRows; i += kThreads) gl[i] = 0.f;
    __syncthreads();
    if (hh == 0 && valid)
        for (int c = 0; c < nc; ++c) {       // (in category order: a token two categories share is added to in a fixed order)
            const int a = arg[row * Cmax + c];
            if (a >= 0 && a < nt) gl[a * kRows + r] += gout[row * T_out + c];
        }
    __syncthreads();

    // ---- gzT = textT glT: lane (r, hh), register reg of tile j holds gz[row r][32 j + rowmap(reg, hh)] --------------------------------
    f32x16 acc[kTiles];
#pragma unroll
    for (int j = 0; j < kTiles; ++j) acc[j] = zero16();
    const float *tb = text + (size_t)b * T * kD;
#pragma unroll 1
    for (int s = 0; s < nt2 / 2; ++s) {
        const int t = 2 * s + hh;
        const float gv = gl[t * kRows + r];
        if (__ballot(gv != 0.f) == 0ull) continue;       // no row of the wave sends anything to these two tokens
        const float *tr = tb + (size_t)(t < nt ? t : nt - 1) * kD + r;
#pragma unroll
        for (int j = 0; j < kTiles; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(tr[32 * j], gv, acc[j], 0, 0, 0);
    }
    if (valid) {
#pragma unroll
        for (int j = 0; j < kTiles; ++j) store_tile(gz + (size_t)row * kD, 32 * j, hh, acc[j]);
    }

    // ---- the block's column sums of gz, one double each ---------------------------------------------------------------------------------
    double *mine = part + (size_t)blockIdx.x * kD;
#pragma unroll
    for (int j = 0; j < kTiles; ++j)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float v = valid ? acc[j][reg] : 0.f;
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (r == 0) mine[32 * j + rowmap(reg, hh)] = (double)v;
        }

    // ---- gxT = WT gzT -------------------------------------------------------------------------------------------------------------------
    if (gx != nullptr) {
#pragma unroll 1
        for (int kt = 0; kt < kTiles; ++kt) {
            f32x16 o = zero16();
            const float *wc = W + 32 * kt + r;
#pragma unroll
            for (int j = 0; j < kTiles; ++j)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    o = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[(size_t)(32 * j + rowmap(reg, hh)) * kD], acc[j][reg], o, 0, 0, 0);
            if (valid) store_tile(gx + (size_t)row * kD, 32 * kt, hh, o);
        }
    }

    // ---- g_b: the last block to arrive adds the blocks' doubles in index order ------------------------------------------------------------
    // (ticket.h's protocol in its older spelling: __threadfence() is a stronger fence, other machine code)
    __threadfence();
    __syncthreads();
    if (lane == 0) {
        __threadfence();
        const unsigned ticket = atomicInc(counter, gridDim.x - 1);       // wraps to 0 behind the last block: ready for the next call
        is_last = ticket == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    // (behind the acquire fence plain loads see the other blocks' doubles, and unlike atomic loads they are issued ahead of
    //  their use: a lane adds four neighbouring columns, block after block)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const double2 *src = reinterpret_cast<const double2 *>(part) + 2 * lane;
#pragma unroll 8
    for (unsigned i = 0; i < gridDim.x; ++i) {
        const double2 a = src[(size_t)i * (kD / 2)], c = src[(size_t)i * (kD / 2) + 1];
        s0 += a.x; s1 += a.y; s2 += c.x; s3 += c.y;
    }
    *reinterpret_cast<float4 *>(g_b + 4 * lane) = make_float4((float)s0, (float)s1, (float)s2, (float)s3);
}

inline long long blocks_of(long long R, int Q) { return (R / Q) * ((Q + kRows - 1) / kRows); }
inline long long max_blocks(long long R) { return R; }      // (Q = 1: a block per row)

// workspace (floats): [the blocks' doubles: 256 per block, sized for the worst dealing][gz R x 256][zira_xty_f32's scratch]
struct Layout {
    size_t part, gz, xty, total;
};
inline Layout layout(long long R)
{
    Layout l;
    l.part = 0;
    l.gz = align4(2 * (size_t)max_blocks(R) * kD);
    l.xty = l.gz + (size_t)R * kD;
    l.total = l.xty + align4(zira_xty_workspace_floats(1, (int)R, kD, kD));
    return l;
}

inline bool bad_shape(long long R, int B, int Q, int T, int T_out, int Cmax)
{
    return R < 1 || R > kMaxR || B < 1 || Q < 1 || R % ((long long)B * Q) != 0 || T < 1 || T > kMaxT || Cmax < 1 || Cmax > kMaxC
           || T_out < 1 || Cmax > T_out;
}

}  // namespace

extern "C" {

size_t zira_cls_linear_workspace_floats(long long R, int D, int T, int Cmax)
{
    if (D != kD || T < 1 || T > kMaxT || Cmax < 1 || Cmax > kMaxC || R < 1 || R > kMaxR) return 0;
    return layout(R).total;
}

int zira_cls_linear_logits_fwd_f32(const float *x, const float *w, const float *bias, const float *text,
                                   const uint8_t *text_token_mask, const uint8_t *cat_token_mask, const int32_t *cat_token_range,
                                   const int32_t *n_cat, const int32_t *n_tok, long long R, int B, int Q, int T, int T_out,
                                   int Cmax, int Tmax, float for_fill, float *out, int32_t *argmax, void *stream)
{
    if (bad_shape(R, B, Q, T, T_out, Cmax) || Tmax < 1 || Tmax > T_out) return -1;
    if (!x || !w || !bias || !text || !text_token_mask || !cat_token_mask || !cat_token_range || !n_cat || !n_tok || !out || !argmax)
        return -1;
    if (misaligned(x) || misaligned(w) || misaligned(bias) || misaligned(text)) return -1;
    hipLaunchKernelGGL(cls_linear_fwd, dim3((unsigned)blocks_of(R, Q)), dim3(kThreads), 0, (hipStream_t)stream, x, w, bias, text,
                       text_token_mask, cat_token_mask, cat_token_range, n_cat, n_tok, B, Q, T, T_out, Cmax, Tmax, for_fill, out,
                       argmax);
    return (int)hipGetLastError();
}

int zira_cls_linear_logits_bwd_f32(const float *grad_out, const int32_t *argmax, const int32_t *n_cat, const int32_t *n_tok,
                                   const float *x, const float *w, const float *text, long long R, int B, int Q, int T, int T_out,
                                   int Cmax, float *gx, float *g_w, float *g_b, float *workspace, uint32_t *counter, void *stream)
{
    if (bad_shape(R, B, Q, T, T_out, Cmax)) return -1;
    if (!grad_out || !argmax || !n_cat || !n_tok || !x || !w || !text || !g_w || !g_b || !workspace || !counter) return -1;
    if (misaligned(x) || misaligned(w) || misaligned(text) || misaligned(gx) || misaligned(g_w) || misaligned(g_b) || misaligned(workspace)) return -1;
    const Layout l = layout(R);
    float *gz = workspace + l.gz;
    hipLaunchKernelGGL(cls_linear_bwd, dim3((unsigned)blocks_of(R, Q)), dim3(kThreads), 0, (hipStream_t)stream, grad_out, argmax,
                       n_cat, n_tok, w, text, B, Q, T, T_out, Cmax, gz, gx, reinterpret_cast<double *>(workspace + l.part), counter,
                       g_b);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return zira_xty_f32(gz, x, 1, (int)R, kD, kD, 0, g_w, workspace + l.xty, stream);        // g_W [256, 256] = gz^T x
}

}  // extern "C"
